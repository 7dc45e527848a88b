// Device image metrics (include/selftok_hip_ext.h): per-image SSIM and mean squared error of a reconstruction against its original,
// in one pass over the two tensors.  The arithmetic of record (tests/image_metrics_cases.py restates it in numpy):
//   SSIM of Wang et al. with the 11-tap separable Gaussian window the caller passes in (fp64), "valid" windows only, population
//   moments, C1 = 0.01^2, C2 = 0.03^2: csrc/ssim_shared.h's tile body (its passes, quotient and sums, every operation in fp64 and rounded on
//   its own) at T = 11 with cov_norm = 1.0, an exact multiplication, on x = (double)recon, y = (double)o, o = px_unit of the original.
//   MSE with evaluate.psnr_each's operations: d = float32(recon) - o and d * d in fp32, summed in fp64.
//   `quantize`: both inputs first become the bytes save_image writes (px_u8 of csrc/u8_shared.h: the reconstruction in its own type, o in
//   fp32), x = byte / 255.0 in fp64, and the squared error is the exact integer sum of (bx - by)^2.
// One workgroup = one 32 x 16 tile of windows of one (image, channel) plane, as ssim_shared.h lays it out (42 x 26 pixels of x and y, five
// 26 x 32 maps).  The tiles of the last row / column also own the 10 border pixels beyond their windows, so the tiles' pixels partition the
// plane and each squared error is summed by exactly one workgroup.  Both sums are reduced in the fixed tree and written as one pair per
// tile; the finish kernel adds an image's pairs in index order.  No atomics: the result is a function of the image alone.
// LDS: 2 * 26 * 42 * 8 + 5 * 26 * 32 * 8 = 50752 bytes (three workgroups per CU, as many as fp32 inputs would give).
#include "common.h"
#include "selftok_hip_ext.h"
#include "ssim_shared.h"
#include "u8_shared.h"

#pragma clang fp contract(off)

namespace selftok {
namespace {

using ssim::TW; using ssim::TH; using ssim::NT;
constexpr int KW = 11, HALO = KW - 1;          // window taps; pixels a tile reads beyond its windows
constexpr int IW = TW + HALO, IH = TH + HALO;  // pixels per tile
constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;

struct Args {
    const void* recon; const void* orig; double* ws;
    int H, W, ntx, nty, orig_signed, quantize;
    double g[ssim::T_MAX];
};

// grid: B * 3 * nty * ntx workgroups, tile column fastest; ws[2 * workgroup + {0: sum of the tile's SSIM values, 1: sum of its pixels' squared errors}]
template <bool RB, bool OB>
__global__ void __launch_bounds__(NT) img_metrics_kernel(Args a)
{
    __shared__ double sx[IH * IW], sy[IH * IW];
    __shared__ double hm[5][IH][TW];
    const int tid = threadIdx.x;
    const ssim::TilePos t = ssim::tile_pos(a.ntx, a.nty, a.H, a.W);
    const int own_w = t.tx == a.ntx - 1 ? a.W - t.x0 : TW, own_h = t.ty == a.nty - 1 ? a.H - t.y0 : TH;      // <= IW, IH: the last tiles own the border

    double sq = 0.0;
    for (int i = tid; i < IH * IW; i += NT) {
        const int r = i / IW, c = i - r * IW;
        const int gy = t.y0 + r < a.H ? t.y0 + r : a.H - 1, gx = t.x0 + c < a.W ? t.x0 + c : a.W - 1;
        const size_t at = t.base + (size_t)gy * a.W + gx;
        const float xr = load_px<RB>(a.recon, at);
        const float v = load_px<OB>(a.orig, at);
        const bool own = r < own_h && c < own_w;                  // then (gy, gx) is not a clamped address
        double xd, yd, e;
        if (a.quantize) {
            const int bx = px_u8<RB>(xr, false), by = px_u8<false>(v, a.orig_signed), d = bx - by;
            xd = (double)bx / 255.0; yd = (double)by / 255.0; e = (double)(d * d);
        } else {
            const float o = px_unit(v, a.orig_signed);
            const float d = xr - o;
            xd = (double)xr; yd = (double)o; e = (double)(d * d);
        }
        if (own) sq += e;
        sx[i] = xd; sy[i] = yd;
    }
    double* red = &hm[0][0][0];
    red[tid] = ssim::tile_ssim<KW>(sx, sy, hm, a.g, 1.0, C1, C2, t.x0, t.y0, a.H, a.W);
    red[NT + tid] = sq;
    ssim::tree_sum<2>(red);                                       // both kinds in one walk of the tree
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

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

size_t selftok_img_metrics_workspace_bytes(int B, int H, int W)
{
    int ntx, nty;
    const long tiles = ssim::plan("img_metrics", B, H, W, KW, &ntx, &nty);
    return (size_t)tiles * B * 2 * sizeof(double);
}

int selftok_img_metrics(const void* recon, int recon_bf16, const void* orig, int orig_bf16, int orig_signed, int quantize, const double* window11_host, double* out,
                        void* workspace, size_t workspace_bytes, int B, int H, int W, hipStream_t stream)
{
    if (!recon || !orig || !window11_host || !out || !workspace) { set_last_error("img_metrics: null pointer"); return SELFTOK_EINVAL; }
    int ntx, nty;
    const long tiles = ssim::plan("img_metrics", B, H, W, KW, &ntx, &nty);
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
