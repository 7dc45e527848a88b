// Device image metrics (include/selftok_hip_ext.h): per-image SSIM and mean squared error of a reconstruction against its original,
// in one pass over the two tensors.  The arithmetic of record (tests/image_metrics_cases.py restates it in numpy):
//   SSIM of Wang et al. with the 11-tap separable Gaussian window the caller passes in (fp64), "valid" windows only, population
//   moments, C1 = 0.01^2, C2 = 0.03^2, every operation in fp64 and rounded on its own (the build passes -ffp-contract=off; the pragma
//   below says it again for this file): horizontal pass of the five maps x, y, x*x, y*y, x*y (taps ascending), vertical pass (taps
//   ascending), the SSIM quotient, the fp64 sum over channels and windows.
//   MSE with evaluate.psnr_each's operations: d = float32(recon) - o and d * d in fp32, summed in fp64.
//   `quantize`: both inputs first become the bytes save_image writes (to_u8_one of csrc/u8_shared.h), x = byte / 255.0
//   in fp64, and the squared error is the exact integer sum of (bx - by)^2.
// One workgroup = one 32 x 16 tile of windows of one (image, channel) plane: the tile's 42 x 26 pixels of x and y go to LDS as fp64 (source
// addresses clamped to the plane, so nothing outside the two tensors is read), the horizontal pass writes five 26 x 32 fp64 maps to LDS,
// the vertical pass runs in registers.  The tiles of the last row / column also own the 10 border pixels beyond their windows, so the
// tiles' pixels partition the plane and each squared error is summed by exactly one workgroup.  Both sums are reduced in a fixed tree and
// written as one pair per tile; the finish kernel adds an image's pairs in index order.  No atomics: the result is a function of the
// image alone.  LDS: 2 * 26 * 42 * 8 + 5 * 26 * 32 * 8 = 50752 bytes (three workgroups per CU, as many as fp32 inputs would give).
#include "common.h"
#include "selftok_hip_ext.h"
#include "u8_shared.h"
#include <stdio.h>

#pragma clang fp contract(off)

namespace selftok {
namespace {

constexpr int KW = 11, HALO = KW - 1;          // window taps; pixels a tile reads beyond its windows
constexpr int TW = 32, TH = 16;                // windows per tile
constexpr int IW = TW + HALO, IH = TH + HALO;  // pixels per tile
constexpr int NT = 256;
constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;

struct Args {
    const void* recon; const void* orig; double* ws;
    int H, W, ntx, nty, orig_signed, quantize;
    double g[KW];
};

// grid: B * 3 * nty * ntx workgroups, tile column fastest; ws[2 * workgroup + {0: sum of the tile's SSIM values, 1: sum of its pixels' squared errors}]
template <bool RB, bool OB>
__global__ void __launch_bounds__(NT) img_metrics_kernel(Args a)
{
    __shared__ double sx[IH * IW], sy[IH * IW];
    __shared__ double hm[5][IH][TW];
    const int tid = threadIdx.x;
    unsigned blk = blockIdx.x;
    const int tx = (int)(blk % (unsigned)a.ntx); blk /= (unsigned)a.ntx;
    const int ty = (int)(blk % (unsigned)a.nty);
    const size_t plane = blk / (unsigned)a.nty;                   // b * 3 + c
    const int x0 = tx * TW, y0 = ty * TH;
    const int own_w = tx == a.ntx - 1 ? a.W - x0 : TW, own_h = ty == a.nty - 1 ? a.H - y0 : TH;      // <= IW, IH: the last tiles own the border
    const size_t base = plane * (size_t)a.H * a.W;

    double sq = 0.0;
    for (int i = tid; i < IH * IW; i += NT) {
        const int r = i / IW, c = i - r * IW;
        const int gy = y0 + r < a.H ? y0 + r : a.H - 1, gx = x0 + c < a.W ? x0 + c : a.W - 1;
        const size_t at = base + (size_t)gy * a.W + gx;
        const float xr = RB ? bf16_to_f32(((const unsigned short*)a.recon)[at]) : ((const float*)a.recon)[at];
        const float v = OB ? bf16_to_f32(((const unsigned short*)a.orig)[at]) : ((const float*)a.orig)[at];
        const float o = a.orig_signed ? (v + 1.0f) / 2.0f : v;
        const bool own = r < own_h && c < own_w;                  // then (gy, gx) is not a clamped address
        double xd, yd, e;
        if (a.quantize) {
            const int bx = to_u8_one<RB>(xr), by = to_u8_one<false>(o), d = bx - by;
            xd = (double)bx / 255.0; yd = (double)by / 255.0; e = (double)(d * d);
        } else {
            const float d = xr - o;
            xd = (double)xr; yd = (double)o; e = (double)(d * d);
        }
        if (own) sq += e;
        sx[i] = xd; sy[i] = yd;
    }
    __syncthreads();

    for (int i = tid; i < IH * TW; i += NT) {                     // horizontal pass: five maps, taps ascending
        const int r = i / TW, c = i % TW;
        const double* px = sx + r * IW + c;
        const double* py = sy + r * IW + c;
        double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
#pragma unroll
        for (int k = 0; k < KW; ++k) {
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
            for (int k = 0; k < KW; ++k) acc += a.g[k] * hm[q][oy + k][ox];
            m[q] = acc;
        }
        const double mux = m[0], muy = m[1];
        const double vx = m[2] - mux * mux, vy = m[3] - muy * muy, vxy = m[4] - mux * muy;
        const double num = (2.0 * mux * muy + C1) * (2.0 * vxy + C2);
        const double den = (mux * mux + muy * muy + C1) * (vx + vy + C2);
        if (y0 + oy < a.H - HALO && x0 + ox < a.W - HALO) ss += num / den;
    }
    __syncthreads();

    double* red = &hm[0][0][0];                                   // fixed tree over the 256 partial sums of each kind
    red[tid] = ss; red[NT + tid] = sq;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) { red[tid] += red[tid + s]; red[NT + tid] += red[NT + tid + s]; }
        __syncthreads();
    }
    if (tid == 0) { a.ws[2 * (size_t)blockIdx.x] = red[0]; a.ws[2 * (size_t)blockIdx.x + 1] = red[NT]; }
}

// one thread per image: its tile pairs in index order -> out[b] = {mean SSIM, MSE}
__global__ void __launch_bounds__(64) img_metrics_finish_kernel(const double* __restrict__ ws, double* __restrict__ out, int B, long tiles, double windows, double sq_div)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double* p = ws + 2 * (size_t)b * tiles;
    double s = 0.0, q = 0.0;
    for (long i = 0; i < tiles; ++i) { s += p[2 * i]; q += p[2 * i + 1]; }
    out[2 * (size_t)b] = s / windows;
    out[2 * (size_t)b + 1] = q / sq_div;
}

// tiles of one image (3 planes), 0 with the error set when the shape is refused
long plan(int B, int H, int W, int* ntx, int* nty)
{
    char msg[200];
    if (B < 1 || H < KW || W < KW) {
        snprintf(msg, sizeof msg, "img_metrics: need B >= 1 and H, W >= 11 (one window), got B %d, %d x %d", B, H, W); set_last_error(msg); return 0;
    }
    const long hw = (long)H * W;
    if (hw >= (1l << 31) / 3 || (long)B > ((1l << 31) - 1) / (3 * hw)) {
        snprintf(msg, sizeof msg, "img_metrics: B * 3 * H * W must stay below 2^31, got B %d, %d x %d", B, H, W); set_last_error(msg); return 0;
    }
    *ntx = (W - HALO + TW - 1) / TW; *nty = (H - HALO + TH - 1) / TH;
    return 3l * *ntx * *nty;
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

size_t selftok_img_metrics_workspace_bytes(int B, int H, int W)
{
    int ntx, nty;
    const long tiles = plan(B, H, W, &ntx, &nty);
    return (size_t)tiles * B * 2 * sizeof(double);
}

int selftok_img_metrics(const void* recon, int recon_bf16, const void* orig, int orig_bf16, int orig_signed, int quantize, const double* window11_host, double* out,
                        void* workspace, size_t workspace_bytes, int B, int H, int W, hipStream_t stream)
{
    if (!recon || !orig || !window11_host || !out || !workspace) { set_last_error("img_metrics: null pointer"); return SELFTOK_EINVAL; }
    int ntx, nty;
    const long tiles = plan(B, H, W, &ntx, &nty);
    if (!tiles) return SELFTOK_EINVAL;
    if (workspace_bytes < (size_t)tiles * B * 2 * sizeof(double)) { set_last_error("img_metrics: workspace smaller than selftok_img_metrics_workspace_bytes"); return SELFTOK_EINVAL; }
    if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)out & 7) != 0) { set_last_error("img_metrics: workspace and out must be 8-byte aligned"); return SELFTOK_EINVAL; }
    Args a{recon, orig, (double*)workspace, H, W, ntx, nty, orig_signed != 0, quantize != 0, {}};
    for (int k = 0; k < KW; ++k) a.g[k] = window11_host[k];
    const unsigned blocks = (unsigned)(tiles * B);                // < 2^31: every tile holds at least one pixel
    if (recon_bf16 && orig_bf16) hipLaunchKernelGGL((img_metrics_kernel<true, true>), dim3(blocks), dim3(NT), 0, stream, a);
    else if (recon_bf16) hipLaunchKernelGGL((img_metrics_kernel<true, false>), dim3(blocks), dim3(NT), 0, stream, a);
    else if (orig_bf16) hipLaunchKernelGGL((img_metrics_kernel<false, true>), dim3(blocks), dim3(NT), 0, stream, a);
    else hipLaunchKernelGGL((img_metrics_kernel<false, false>), dim3(blocks), dim3(NT), 0, stream, a);
    const double pixels = 3.0 * (double)H * (double)W, windows = 3.0 * (double)(H - HALO) * (double)(W - HALO);
    hipLaunchKernelGGL(img_metrics_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, (const double*)workspace, out, B, tiles, windows,
                       quantize ? 65025.0 * pixels : pixels);
    return check_launch("img_metrics kernels");
}

}  // extern "C"
