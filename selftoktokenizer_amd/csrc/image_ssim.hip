// Device SSIM with a caller-chosen window and moment convention (include/selftok_hip_ext.h: selftok_img_ssim): the mean SSIM of every
// image of a batch for T separable window taps (T odd, 3 .. 11, fp64, from the host), a covariance normalisation `cov_norm` (1 for population
// moments, T^2 / (T^2 - 1) for scikit-image's use_sample_covariance=True) and a data range of 1 (operands on [0, 1]) or 2 (operands on [-1, 1]).
// The arithmetic of record (tests/ssim_variant_cases.py restates it in numpy), fp64 throughout, every operation rounded on its own (the
// build passes -ffp-contract=off; the pragma below says it again for this file):
//   operands: signed_range == 0: x = (double)r, y = (double)o with o = orig_signed ? (v + 1.0f) / 2.0f : v in fp32 -- csrc/image_metrics.hip's own
//             expressions; signed_range != 0: x = 2.0 * (double)r - 1.0, y = orig_signed ? (double)v : 2.0 * (double)v - 1.0.
//             quantize: both first become the bytes save_image writes (to_u8_one; the original from o), p = (double)byte / 255.0, and the operand is p
//             or 2.0 * p - 1.0.
//   ux, uy, uxx, uyy, uxy: horizontal pass of x, y, x*x, y*y, x*y (taps ascending, from 0.0), then the vertical pass (taps ascending, from 0.0)
//   vx = cov_norm * (uxx - ux * ux), vy likewise, vxy = cov_norm * (uxy - ux * uy)
//   S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2)), C1 = (0.01 R)^2, C2 = (0.03 R)^2, R = 1 or 2
//   out[b] = the fp64 sum over the three channels and the (H - T + 1) x (W - T + 1) "valid" windows, divided by their number.
// This is the fp64 form; scikit-image >= 0.19 computes float32 input in float32, which this entry does not imitate.
// The tile scheme is image_metrics.hip's: one workgroup = one 32 x 16 tile of windows of one (image, channel) plane, its (32 + T - 1) x
// (16 + T - 1) pixels in LDS as fp64 (source addresses clamped to the plane), five horizontally filtered maps in LDS, the vertical pass in
// registers, a fixed tree over the 256 partial sums, one fp64 per tile; the finish kernel adds an image's tiles in index order.  With T = 11,
// cov_norm = 1.0 (an exact multiplication) and signed_range = 0 every operation and every order is that of selftok_img_metrics' SSIM: the same
// bits.  No atomics: out[b] is a function of image b alone.  LDS at T = 11: 50752 bytes.
#include "common.h"
#include "selftok_hip_ext.h"
#include "u8_shared.h"
#include <stdio.h>

#pragma clang fp contract(off)

namespace selftok {
namespace {

constexpr int TW = 32, TH = 16;                // windows per tile
constexpr int NT = 256;
constexpr int T_MIN = 3, T_MAX = 11;

struct Args {
    const void* recon; const void* orig; double* ws;
    int H, W, ntx, nty, recon_bf16, orig_bf16, orig_signed, quantize, signed_range;
    double cov_norm, c1, c2;
    double g[T_MAX];
};

// grid: B * 3 * nty * ntx workgroups, tile column fastest; ws[workgroup] = the sum of the tile's SSIM values
template <int T>
__global__ void __launch_bounds__(NT) img_ssim_kernel(Args a)
{
    constexpr int HALO = T - 1, IW = TW + HALO, IH = TH + HALO;
    __shared__ double sx[IH * IW], sy[IH * IW];
    __shared__ double hm[5][IH][TW];
    const int tid = threadIdx.x;
    unsigned blk = blockIdx.x;
    const int tx = (int)(blk % (unsigned)a.ntx); blk /= (unsigned)a.ntx;
    const int ty = (int)(blk % (unsigned)a.nty);
    const size_t plane = blk / (unsigned)a.nty;                   // b * 3 + c
    const int x0 = tx * TW, y0 = ty * TH;
    const size_t base = plane * (size_t)a.H * a.W;

    for (int i = tid; i < IH * IW; i += NT) {
        const int r = i / IW, c = i - r * IW;
        const int gy = y0 + r < a.H ? y0 + r : a.H - 1, gx = x0 + c < a.W ? x0 + c : a.W - 1;      // clamped: a window that reads such a pixel is not counted
        const size_t at = base + (size_t)gy * a.W + gx;
        const float xr = a.recon_bf16 ? bf16_to_f32(((const unsigned short*)a.recon)[at]) : ((const float*)a.recon)[at];
        const float v = a.orig_bf16 ? bf16_to_f32(((const unsigned short*)a.orig)[at]) : ((const float*)a.orig)[at];
        double xd, yd;
        if (a.quantize) {
            const float o = a.orig_signed ? (v + 1.0f) / 2.0f : v;
            const int bx = a.recon_bf16 ? to_u8_one<true>(xr) : to_u8_one<false>(xr), by = to_u8_one<false>(o);
            xd = (double)bx / 255.0; yd = (double)by / 255.0;
            if (a.signed_range) { xd = 2.0 * xd - 1.0; yd = 2.0 * yd - 1.0; }
        } else if (a.signed_range) {
            xd = 2.0 * (double)xr - 1.0;
            yd = a.orig_signed ? (double)v : 2.0 * (double)v - 1.0;
        } else {
            const float o = a.orig_signed ? (v + 1.0f) / 2.0f : v;
            xd = (double)xr; yd = (double)o;
        }
        sx[i] = xd; sy[i] = yd;
    }
    __syncthreads();

    for (int i = tid; i < IH * TW; i += NT) {                     // horizontal pass: five maps, taps ascending
        const int r = i / TW, c = i % TW;
        const double* px = sx + r * IW + c;
        const double* py = sy + r * IW + c;
        double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const double x = px[k], y = py[k], g = a.g[k];
            hx += g * x; hy += g * y; hxx += g * (x * x); hyy += g * (y * y); hxy += g * (x * y);
        }
        hm[0][r][c] = hx; hm[1][r][c] = hy; hm[2][r][c] = hxx; hm[3][r][c] = hyy; hm[4][r][c] = hxy;
    }
    __syncthreads();

    double ss = 0.0;
#pragma unroll
    for (int j = 0; j < TH * TW / NT; ++j) {                      // vertical pass in registers: window rows tid / 32 and tid / 32 + 8
        const int oy = (tid >> 5) + j * (NT / TW), ox = tid & (TW - 1);
        double m[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < T; ++k) acc += a.g[k] * hm[q][oy + k][ox];
            m[q] = acc;
        }
        const double mux = m[0], muy = m[1];
        const double vx = a.cov_norm * (m[2] - mux * mux), vy = a.cov_norm * (m[3] - muy * muy), vxy = a.cov_norm * (m[4] - mux * muy);
        const double num = (2.0 * mux * muy + a.c1) * (2.0 * vxy + a.c2);
        const double den = (mux * mux + muy * muy + a.c1) * (vx + vy + a.c2);
        if (y0 + oy < a.H - HALO && x0 + ox < a.W - HALO) ss += num / den;
    }
    __syncthreads();

    double* red = &hm[0][0][0];                                   // fixed tree over the 256 partial sums (5 * IH * TW >= 2880 doubles)
    red[tid] = ss;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) a.ws[blockIdx.x] = red[0];
}

// one thread per image: its tiles in index order -> out[b] = mean SSIM
__global__ void __launch_bounds__(64) img_ssim_finish_kernel(const double* __restrict__ ws, double* __restrict__ out, int B, long tiles, double windows)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double* p = ws + (size_t)b * tiles;
    double s = 0.0;
    for (long i = 0; i < tiles; ++i) s += p[i];
    out[b] = s / windows;
}

// tiles of one image (3 planes), 0 with the error set when the shape or the window is refused
long plan(int B, int H, int W, int taps, int* ntx, int* nty)
{
    char msg[200];
    if (taps < T_MIN || taps > T_MAX || taps % 2 == 0) {
        snprintf(msg, sizeof msg, "img_ssim: need an odd number of window taps, 3 <= taps <= 11, got %d", taps); set_last_error(msg); return 0;
    }
    if (B < 1 || H < taps || W < taps) {
        snprintf(msg, sizeof msg, "img_ssim: need B >= 1 and H, W >= taps = %d (one window), got B %d, %d x %d", taps, B, H, W); set_last_error(msg); return 0;
    }
    const long hw = (long)H * W;
    if (hw >= (1l << 31) / 3 || (long)B > ((1l << 31) - 1) / (3 * hw)) {
        snprintf(msg, sizeof msg, "img_ssim: B * 3 * H * W must stay below 2^31, got B %d, %d x %d", B, H, W); set_last_error(msg); return 0;
    }
    const int halo = taps - 1;
    *ntx = (W - halo + TW - 1) / TW; *nty = (H - halo + TH - 1) / TH;
    return 3l * *ntx * *nty;
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

size_t selftok_img_ssim_workspace_bytes(int B, int H, int W, int taps)
{
    int ntx, nty;
    const long tiles = plan(B, H, W, taps, &ntx, &nty);
    return (size_t)tiles * B * sizeof(double);
}

int selftok_img_ssim(const void* recon, int recon_bf16, const void* orig, int orig_bf16, int orig_signed, int quantize, const double* window_host, int taps,
                     double cov_norm, int signed_range, double* out, void* workspace, size_t workspace_bytes, int B, int H, int W, hipStream_t stream)
{
    if (!recon || !orig || !window_host || !out || !workspace) { set_last_error("img_ssim: null pointer"); return SELFTOK_EINVAL; }
    int ntx, nty;
    const long tiles = plan(B, H, W, taps, &ntx, &nty);
    if (!tiles) return SELFTOK_EINVAL;
    if (!(cov_norm > 0.0) || cov_norm > 2.0) { set_last_error("img_ssim: need 0 < cov_norm <= 2 (1 for population moments, T^2 / (T^2 - 1) for sample moments)"); return SELFTOK_EINVAL; }
    if (workspace_bytes < (size_t)tiles * B * sizeof(double)) { set_last_error("img_ssim: workspace smaller than selftok_img_ssim_workspace_bytes"); return SELFTOK_EINVAL; }
    if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)out & 7) != 0) { set_last_error("img_ssim: workspace and out must be 8-byte aligned"); return SELFTOK_EINVAL; }
    const double R = signed_range ? 2.0 : 1.0;
    Args a{recon, orig, (double*)workspace, H, W, ntx, nty, recon_bf16 != 0, orig_bf16 != 0, orig_signed != 0, quantize != 0, signed_range != 0,
           cov_norm, (0.01 * R) * (0.01 * R), (0.03 * R) * (0.03 * R), {}};
    for (int k = 0; k < taps; ++k) a.g[k] = window_host[k];
    const dim3 grid((unsigned)(tiles * B));                       // < 2^31: every tile holds at least one pixel
    switch (taps) {
    case 3: hipLaunchKernelGGL(img_ssim_kernel<3>, grid, dim3(NT), 0, stream, a); break;
    case 5: hipLaunchKernelGGL(img_ssim_kernel<5>, grid, dim3(NT), 0, stream, a); break;
    case 7: hipLaunchKernelGGL(img_ssim_kernel<7>, grid, dim3(NT), 0, stream, a); break;
    case 9: hipLaunchKernelGGL(img_ssim_kernel<9>, grid, dim3(NT), 0, stream, a); break;
    default: hipLaunchKernelGGL(img_ssim_kernel<11>, grid, dim3(NT), 0, stream, a); break;
    }
    const double windows = 3.0 * (double)(H - (taps - 1)) * (double)(W - (taps - 1));
    hipLaunchKernelGGL(img_ssim_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, (const double*)workspace, out, B, tiles, windows);
    return check_launch("img_ssim kernels");
}

}  // extern "C"
