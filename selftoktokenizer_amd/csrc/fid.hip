// rFID (FID InceptionV3, pool3 = 2048 features) on the device (include/selftok_hip_ext.h): the stages selftoktokenizer_amd/fid.py
// (FID_DEFINITION, InceptionNet) chains, and the fp64 mean / covariance of a feature matrix.  tests/fid_cases.py restates the network in
// torch-CPU fp64 and the statistics in numpy fp64.  Activations are channels-last fp32 [N, H, W, C]; a block's branches write their
// channel slices of ONE concatenated map (row stride `ldo`, first channel `co_off`): there is no concatenation pass.
//
// Convolution: csrc/conv_f32_shared.h's tile body and host side, the ones selftok_lpips_conv2d_f32 runs -- the arithmetic of record at the
// top of csrc/lpips.hip (eight fmaf chains by k mod 16 on v_mfma_f32_32x32x2_f32, fixed tree, one bias addition, ReLU), with pad_h / pad_w
// per axis and the slice.
// Pool (3 x 3): max / stride 2 / no padding, max / stride 1 / pad 1, average / stride 1 / pad 1 with the number of in-image taps as the
//   divisor -- three instances of csrc/pool_shared.h's body, which states the rule.
// Input: x = float32(v) * 2 - 1 of a [0, 1] image, a signed image as it is; quantize: byte / 255 * 2 - 1 of the byte save_image writes
//   (px_u8 of csrc/u8_shared.h: an unsigned image in its own type, a signed one from (v + 1) / 2 in fp32).  With tap tables
//   (i0, i1, lambda per output row and column, built on the host in fp64) a bilinear resize of the converted values, each operation
//   rounded to fp32 on its own: top = a + lx * (b - a), bot = c + lx * (d - c) (horizontal pairs first), x = top + ly * (bot - top).
// Spatial mean: s = +0.0f, s = s + f[p] for the pixels p in index order, then s / (float)npix, per image and channel.
// Statistics (fp64 from the fp32 features on; every fma spelled out, nothing else contracted):
//   rows are walked in chunks of 256 (chunk c = rows 256 c .. 256 c + 255).  Within a chunk a value is accumulated from +0.0 in ascending
//   row order; the chunk values are combined by the pairwise tree of a binary counter (chunk_tree below): the sum of 2^(l + 1)
//   consecutive chunks is (earlier 2^l) + (later 2^l), and the blocks left over by the binary expansion of the chunk count are added from
//   the latest (smallest) to the earliest, t = block + t.  mu[d] = tree of (chunk sums of (double)x[n, d]) / N.
//   sigma[i, j] = tree of (chunk chains c = fma(a_ni, a_nj, c), a_nd = (double)x[n, d] - mu[d]) / (N - 1).  One workgroup owns a 16 x 16
//   tile of the upper triangle and writes it and its mirror image: sigma is exactly symmetric (in a diagonal tile (i, j) and (j, i) are
//   the same products in the same order).  No atomics; the result is a function of X alone.
#include "common.h"
#include "conv_f32_shared.h"
#include "pool_shared.h"
#include "u8_shared.h"
#include "chunk_tree.h"
#include "selftok_hip_ext.h"
#include <stdio.h>

#pragma clang fp contract(off)

namespace selftok {
namespace {

using conv_f32::NT; using conv_f32::ConvArgs;

template <bool VEC>
__global__ void __launch_bounds__(NT) fid_conv_kernel(ConvArgs a)
{
    conv_f32::conv_tile<VEC>(a);
}

// mode 0: max, stride 2, pad 0; 1: max, stride 1, pad 1; 2: average, stride 1, pad 1, in-image divisor
template <int MODE>
__global__ void __launch_bounds__(NT) fid_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, int PH, int PW, int ldo, int co_off,
                                                      long total)
{
    pool::pool_element<3, MODE == 0 ? 2 : 1, MODE == 0 ? 0 : 1, MODE == 2>(in, out, H, W, C, PH, PW, ldo, co_off, total);
}

struct InputArgs {
    const void* src; float* out; const int* ytab; const int* xtab;
    int B, H, W, OH, OW, is_signed, quantize;
    long total;                                                   // B * OH * OW * 3
};

template <bool BF>
__device__ __forceinline__ float fid_convert(const InputArgs& a, size_t at)
{
    const float v = load_px<BF>(a.src, at);
    if (a.quantize) {
        const unsigned char b = a.is_signed ? px_u8<false>(v, true) : px_u8<BF>(v, false);        // an unsigned image in its own type: this entry's convention
        return (float)b / 255.0f * 2.0f - 1.0f;
    }
    return a.is_signed ? v : v * 2.0f - 1.0f;
}

// src [B, 3, H, W] -> out [B, OH, OW, 3]; ytab = i0[OH], i1[OH], lambda bits[OH] (xtab likewise), or both NULL: OH = H, OW = W, no resize
template <bool BF>
__global__ void __launch_bounds__(NT) fid_input_kernel(InputArgs a)
{
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= a.total) return;
    const int c = (int)(i % 3);
    long p = i / 3;
    const int ox = (int)(p % a.OW); p /= a.OW;
    const int oy = (int)(p % a.OH);
    const long n = p / a.OH;
    const size_t plane = ((size_t)n * 3 + c) * a.H * a.W;
    if (!a.ytab) { a.out[i] = fid_convert<BF>(a, plane + (size_t)oy * a.W + ox); return; }
    const int hi_y = a.H - 1, hi_x = a.W - 1;
    const int y0 = min(max(a.ytab[oy], 0), hi_y), y1 = min(max(a.ytab[a.OH + oy], 0), hi_y);      // a table cannot point outside the image
    const int x0 = min(max(a.xtab[ox], 0), hi_x), x1 = min(max(a.xtab[a.OW + ox], 0), hi_x);
    const float ly = __int_as_float(a.ytab[2 * a.OH + oy]), lx = __int_as_float(a.xtab[2 * a.OW + ox]);
    const float va = fid_convert<BF>(a, plane + (size_t)y0 * a.W + x0), vb = fid_convert<BF>(a, plane + (size_t)y0 * a.W + x1);
    const float vc = fid_convert<BF>(a, plane + (size_t)y1 * a.W + x0), vd = fid_convert<BF>(a, plane + (size_t)y1 * a.W + x1);
    const float top = va + lx * (vb - va);
    const float bot = vc + lx * (vd - vc);
    a.out[i] = top + ly * (bot - top);
}

// in [N, npix, C] -> out [N, C]
__global__ void __launch_bounds__(NT) fid_mean_kernel(const float* __restrict__ in, float* __restrict__ out, int npix, int C, long total)
{
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const long n = i / C;
    const float* src = in + (size_t)n * npix * C + c;
    float s = 0.0f;
    for (int p = 0; p < npix; ++p) s = s + src[(size_t)p * C];
    out[i] = s / (float)npix;
}

// ---- statistics ----
constexpr int SCH = 256;                                          // rows per chunk (csrc/chunk_tree.h: the tree across chunks)
constexpr int ST = 16, SSUB = 32;                                 // covariance tile side; rows staged per step

// grid (ceil(D / 64), chunks): ws[chunk * D + d] = the chunk's sum of column d
__global__ void __launch_bounds__(64) fid_colsum_kernel(const float* __restrict__ x, double* __restrict__ ws, int N, int D)
{
    const int d = blockIdx.x * 64 + threadIdx.x;
    if (d >= D) return;
    const int n0 = blockIdx.y * SCH, n1 = min(n0 + SCH, N);
    double s = 0.0;
    for (int n = n0; n < n1; ++n) s = s + (double)x[(size_t)n * D + d];
    ws[(size_t)blockIdx.y * D + d] = s;
}

__global__ void __launch_bounds__(64) fid_mu_kernel(const double* __restrict__ ws, double* __restrict__ mu, int N, int D, int chunks)
{
    const int d = blockIdx.x * 64 + threadIdx.x;
    if (d >= D) return;
    chunk_tree t; t.init();
    for (int c = 0; c < chunks; ++c) t.push(ws[(size_t)c * D + d]);
    mu[d] = t.total() / (double)N;
}

// grid (D / 16, D / 16), tiles below the diagonal return at once; thread (r, c) owns sigma[ti * 16 + r, tj * 16 + c]
__global__ void __launch_bounds__(NT) fid_cov_kernel(const float* __restrict__ x, const double* __restrict__ mu, double* __restrict__ sigma, int N, int D)
{
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    __shared__ double As[SSUB][ST], Bs[SSUB][ST];
    const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
    const int lr = r, lc = c;                                     // load role: rows lr and lr + 16 of a step, column lc of both sides
    const double mu_i = mu[ti * ST + lc], mu_j = mu[tj * ST + lc];
    const float* xi = x + ti * ST + lc;
    const float* xj = x + tj * ST + lc;
    chunk_tree t; t.init();
    for (int n0 = 0; n0 < N; n0 += SCH) {
        double acc = 0.0;
        for (int s0 = n0; s0 < min(n0 + SCH, N); s0 += SSUB) {
            __syncthreads();                                      // the previous step's reads are done
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int n = s0 + lr + 16 * h;
                const bool in = n < min(n0 + SCH, N);             // a row past the chunk is a pair of exact zeros: fma(0, 0, c) = c
                As[lr + 16 * h][lc] = in ? (double)xi[(size_t)n * D] - mu_i : 0.0;
                Bs[lr + 16 * h][lc] = in ? (double)xj[(size_t)n * D] - mu_j : 0.0;
            }
            __syncthreads();
#pragma unroll 8
            for (int n = 0; n < SSUB; ++n) acc = fma(As[n][r], Bs[n][c], acc);
        }
        t.push(acc);
    }
    const double v = t.total() / (double)(N - 1);
    const size_t i = (size_t)ti * ST + r, j = (size_t)tj * ST + c;
    sigma[i * D + j] = v;
    if (ti != tj) sigma[j * D + i] = v;
}

bool fail(const char* msg) { set_last_error(msg); return false; }

constexpr long LIM = 1l << 31;

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

int selftok_fid_conv2d_f32(const float* in, const float* packed, const float* bias, float* out, int N, int H, int W, int Cin, int Cout,
                           int KH, int KW, int stride, int pad_h, int pad_w, int ldo, int co_off, int relu, hipStream_t stream)
{
    ConvArgs a;
    dim3 grid;
    if (!conv_f32::conv_plan("fid_conv2d", in, packed, bias, out, N, H, W, Cin, Cout, KH, KW, stride, pad_h, pad_w, ldo, co_off, relu, &a, &grid)) return SELFTOK_EINVAL;
    if (Cin % 4 == 0) hipLaunchKernelGGL(fid_conv_kernel<true>, grid, dim3(NT), 0, stream, a);
    else hipLaunchKernelGGL(fid_conv_kernel<false>, grid, dim3(NT), 0, stream, a);
    return check_launch("fid_conv_kernel");
}

int selftok_fid_pool3_f32(const float* in, float* out, int N, int H, int W, int C, int mode, int ldo, int co_off, hipStream_t stream)
{
    if (mode < 0 || mode > 2) {
        char msg[160];
        snprintf(msg, sizeof msg, "fid_pool3: need mode 0 (max / 2, H, W >= 3), 1 (max, pad 1) or 2 (average, pad 1), got mode %d", mode);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    int PH, PW;
    long total;
    if (!(mode == 0 ? pool::check<3, 2, 0>("fid_pool3", in, out, N, H, W, C, ldo, co_off, &PH, &PW, &total)
                    : pool::check<3, 1, 1>("fid_pool3", in, out, N, H, W, C, ldo, co_off, &PH, &PW, &total))) return SELFTOK_EINVAL;
    const dim3 grid((unsigned)((total + NT - 1) / NT));
    if (mode == 0) hipLaunchKernelGGL(fid_pool_kernel<0>, grid, dim3(NT), 0, stream, in, out, H, W, C, PH, PW, ldo, co_off, total);
    else if (mode == 1) hipLaunchKernelGGL(fid_pool_kernel<1>, grid, dim3(NT), 0, stream, in, out, H, W, C, PH, PW, ldo, co_off, total);
    else hipLaunchKernelGGL(fid_pool_kernel<2>, grid, dim3(NT), 0, stream, in, out, H, W, C, PH, PW, ldo, co_off, total);
    return check_launch("fid_pool_kernel");
}

int selftok_fid_input(const void* src, int src_bf16, int src_signed, int quantize, float* out, int B, int H, int W, int OH, int OW,
                      const int* ytab, const int* xtab, hipStream_t stream)
{
    if (!src || !out) { set_last_error("fid_input: null pointer"); return SELFTOK_EINVAL; }
    char msg[240];
    if ((ytab == nullptr) != (xtab == nullptr)) { set_last_error("fid_input: the row and the column tap table go together"); return SELFTOK_EINVAL; }
    if (B < 1 || H < 1 || W < 1 || OH < 1 || OW < 1 || (!ytab && (OH != H || OW != W))) {
        snprintf(msg, sizeof msg, "fid_input: need B, H, W, OH, OW >= 1 and, without tap tables, OH x OW = H x W, got B %d, %d x %d -> %d x %d", B, H, W, OH, OW);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if ((long)H * W >= LIM / 3 || (long)B >= LIM / (3l * H * W) || (long)OH * OW >= LIM / 3 || (long)B >= LIM / (3l * OH * OW)) {
        snprintf(msg, sizeof msg, "fid_input: B * 3 * H * W of the source and of the output must stay below 2^31, got B %d, %d x %d -> %d x %d", B, H, W, OH, OW);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    InputArgs a{src, out, ytab, xtab, B, H, W, OH, OW, src_signed != 0, quantize != 0, 3l * B * OH * OW};
    const dim3 grid((unsigned)((a.total + NT - 1) / NT));
    if (src_bf16) hipLaunchKernelGGL(fid_input_kernel<true>, grid, dim3(NT), 0, stream, a);
    else hipLaunchKernelGGL(fid_input_kernel<false>, grid, dim3(NT), 0, stream, a);
    return check_launch("fid_input_kernel");
}

int selftok_fid_spatial_mean_f32(const float* in, float* out, int N, int npix, int C, hipStream_t stream)
{
    if (!in || !out) { set_last_error("fid_spatial_mean: null pointer"); return SELFTOK_EINVAL; }
    char msg[200];
    if (N < 1 || npix < 1 || C < 1 || (long)npix >= LIM / C || (long)N >= LIM / ((long)npix * C)) {
        snprintf(msg, sizeof msg, "fid_spatial_mean: need N, npix, C >= 1 and N * npix * C below 2^31, got N %d, npix %d, C %d", N, npix, C);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    const long total = (long)N * C;
    hipLaunchKernelGGL(fid_mean_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, stream, in, out, npix, C, total);
    return check_launch("fid_mean_kernel");
}

size_t selftok_fid_stats_workspace_bytes(int N, int D)
{
    char msg[200];
    if (N < 2 || D < 16 || D % 16 != 0 || D > 16 * 65535 || ((long)N + SCH - 1) / SCH > 65535 || (long)N >= LIM / D) {
        snprintf(msg, sizeof msg, "fid_stats: need 2 <= N <= 256 * 65535, D a multiple of 16 up to 16 * 65535 and N * D below 2^31, got N %d, D %d", N, D);
        set_last_error(msg); return 0;
    }
    return (size_t)(((long)N + SCH - 1) / SCH) * (size_t)D * sizeof(double);
}

int selftok_fid_stats(const float* x, double* mu, double* sigma, void* workspace, size_t workspace_bytes, int N, int D, hipStream_t stream)
{
    if (!x || !mu || !sigma || !workspace) { set_last_error("fid_stats: null pointer"); return SELFTOK_EINVAL; }
    const size_t need = selftok_fid_stats_workspace_bytes(N, D);
    if (!need) return SELFTOK_EINVAL;
    if (workspace_bytes < need) { set_last_error("fid_stats: workspace smaller than selftok_fid_stats_workspace_bytes"); return SELFTOK_EINVAL; }
    if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)mu & 7) != 0 || ((uintptr_t)sigma & 7) != 0 || ((uintptr_t)x & 3) != 0) {
        set_last_error("fid_stats: workspace, mu and sigma must be 8-byte aligned, x 4-byte aligned"); return SELFTOK_EINVAL;
    }
    const int chunks = (N + SCH - 1) / SCH;
    hipLaunchKernelGGL(fid_colsum_kernel, dim3((D + 63) / 64, chunks), dim3(64), 0, stream, x, (double*)workspace, N, D);
    hipLaunchKernelGGL(fid_mu_kernel, dim3((D + 63) / 64), dim3(64), 0, stream, (const double*)workspace, mu, N, D, chunks);
    hipLaunchKernelGGL(fid_cov_kernel, dim3(D / ST, D / ST), dim3(NT), 0, stream, x, (const double*)mu, sigma, N, D);
    return check_launch("fid_stats kernels");
}

}  // extern "C"
