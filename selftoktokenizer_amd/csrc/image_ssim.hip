// Device SSIM with a caller-chosen window and moment convention (include/selftok_hip_ext.h: selftok_img_ssim): the mean SSIM of every
// image of a batch for T separable window taps (T odd, 3 .. 11, fp64, from the host), a covariance normalisation `cov_norm` (1 for population
// moments, T^2 / (T^2 - 1) for scikit-image's use_sample_covariance=True) and a data range of 1 (operands on [0, 1]) or 2 (operands on [-1, 1]).
// The arithmetic of record from the operands on (the two passes, the moments, the quotient with C1 = (0.01 R)^2, C2 = (0.03 R)^2, the sums), the tile
// scheme and its LDS are csrc/ssim_shared.h's, the body selftok_img_metrics runs too; tests/ssim_variant_cases.py restates all of it in numpy.
// What is this file's own, every operation rounded on its own (the build passes -ffp-contract=off; the pragma below says it again):
//   operands: signed_range == 0: x = (double)r, y = (double)o with o = orig_signed ? (v + 1.0f) / 2.0f : v in fp32 -- csrc/image_metrics.hip's
//             operands; signed_range != 0: x = 2.0 * (double)r - 1.0, y = orig_signed ? (double)v : 2.0 * (double)v - 1.0.
//             quantize: both first become the bytes save_image writes (px_u8 of csrc/u8_shared.h; the original from o), p = (double)byte / 255.0, and
//             the operand is p or 2.0 * p - 1.0.
//   out[b] = the sum of image b's tiles in index order, divided by the number of windows.
// This is the fp64 form; scikit-image >= 0.19 computes float32 input in float32, which this entry does not imitate.
// With T = 11, cov_norm = 1.0 (an exact multiplication) and signed_range = 0 every operation and every order is that of selftok_img_metrics' SSIM: the
// same bits.  No atomics: out[b] is a function of image b alone.  LDS at T = 11: 50752 bytes.
#include "common.h"
#include "selftok_hip_ext.h"
#include "ssim_shared.h"
#include "u8_shared.h"

#pragma clang fp contract(off)

namespace selftok {
namespace {

using ssim::TW; using ssim::TH; using ssim::NT; using ssim::T_MAX;

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
    const ssim::TilePos t = ssim::tile_pos(a.ntx, a.nty, a.H, a.W);

    for (int i = tid; i < IH * IW; i += NT) {
        const int r = i / IW, c = i - r * IW;
        const int gy = t.y0 + r < a.H ? t.y0 + r : a.H - 1, gx = t.x0 + c < a.W ? t.x0 + c : a.W - 1;      // clamped: a window that reads such a pixel is not counted
        const size_t at = t.base + (size_t)gy * a.W + gx;
        const float xr = a.recon_bf16 ? load_px<true>(a.recon, at) : load_px<false>(a.recon, at);
        const float v = a.orig_bf16 ? load_px<true>(a.orig, at) : load_px<false>(a.orig, at);
        double xd, yd;
        if (a.quantize) {
            const int bx = a.recon_bf16 ? px_u8<true>(xr, false) : px_u8<false>(xr, false), by = px_u8<false>(v, a.orig_signed);
            xd = (double)bx / 255.0; yd = (double)by / 255.0;
            if (a.signed_range) { xd = 2.0 * xd - 1.0; yd = 2.0 * yd - 1.0; }
        } else if (a.signed_range) {
            xd = 2.0 * (double)xr - 1.0;
            yd = a.orig_signed ? (double)v : 2.0 * (double)v - 1.0;
        } else {
            xd = (double)xr; yd = (double)px_unit(v, a.orig_signed);
        }
        sx[i] = xd; sy[i] = yd;
    }
    double* red = &hm[0][0][0];                                   // 5 * IH * TW >= 2880 doubles
    red[tid] = ssim::tile_ssim<T>(sx, sy, hm, a.g, a.cov_norm, a.c1, a.c2, t.x0, t.y0, a.H, a.W);
    ssim::tree_sum<1>(red);
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

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

size_t selftok_img_ssim_workspace_bytes(int B, int H, int W, int taps)
{
    int ntx, nty;
    const long tiles = ssim::plan("img_ssim", B, H, W, taps, &ntx, &nty);
    return (size_t)tiles * B * sizeof(double);
}

int selftok_img_ssim(const void* recon, int recon_bf16, const void* orig, int orig_bf16, int orig_signed, int quantize, const double* window_host, int taps,
                     double cov_norm, int signed_range, double* out, void* workspace, size_t workspace_bytes, int B, int H, int W, hipStream_t stream)
{
    if (!recon || !orig || !window_host || !out || !workspace) { set_last_error("img_ssim: null pointer"); return SELFTOK_EINVAL; }
    int ntx, nty;
    const long tiles = ssim::plan("img_ssim", B, H, W, taps, &ntx, &nty);
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
