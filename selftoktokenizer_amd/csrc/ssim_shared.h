// The SSIM tile body shared by csrc/image_metrics.hip (selftok_img_metrics) and csrc/image_ssim.hip (selftok_img_ssim): ONE body, so both entries
// have the same arithmetic of record and, at T = 11 with cov_norm = 1.0 (an exact multiplication) and data range 1, the same bits.
// The arithmetic of record (tests/image_metrics_cases.py and tests/ssim_variant_cases.py restate it in numpy), fp64 throughout, every operation
// rounded on its own (the build passes -ffp-contract=off; the pragma of the including file says it again), on operands x, y the caller has
// already converted:
//   ux, uy, uxx, uyy, uxy: horizontal pass of x, y, x*x, y*y, x*y (taps ascending, from 0.0), then the vertical pass (taps ascending, from 0.0)
//   vx = cov_norm * (uxx - ux * ux), vy likewise, vxy = cov_norm * (uxy - ux * uy)
//   S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2)), C1 = (0.01 R)^2, C2 = (0.03 R)^2 for a data range R
//   the fp64 sum over the three channels and the (H - T + 1) x (W - T + 1) "valid" windows, divided by their number.
// The tile scheme: one workgroup (256 threads) = one 32 x 16 tile of windows of one (image, channel) plane, its (32 + T - 1) x (16 + T - 1)
// pixels in LDS as fp64 (the caller fills them from source addresses clamped to the plane, so nothing outside the tensors is read), five
// horizontally filtered maps in LDS, the vertical pass in registers, a fixed tree over the 256 partial sums, one value per tile; the caller's
// finish kernel adds an image's tiles in index order.  Nothing is added out of order: the result is a function of the image alone.
// LDS: 8 * (2 * (15 + T) * (31 + T) + 5 * (15 + T) * 32) bytes, 50752 at T = 11 (three workgroups per CU).
#pragma once
#include "common.h"
#include <stdio.h>

namespace selftok {
namespace ssim {

constexpr int TW = 32, TH = 16;                // windows per tile
constexpr int NT = 256;
constexpr int T_MIN = 3, T_MAX = 11;

// a workgroup's tile: blockIdx.x = (plane * nty + ty) * ntx + tx, tile column fastest
struct TilePos {
    int x0, y0, tx, ty;
    size_t base;                                                   // element offset of the (image, channel) plane b * 3 + c
};

__device__ __forceinline__ TilePos tile_pos(int ntx, int nty, int H, int W)
{
    unsigned blk = blockIdx.x;
    TilePos p;
    p.tx = (int)(blk % (unsigned)ntx); blk /= (unsigned)ntx;
    p.ty = (int)(blk % (unsigned)nty);
    p.x0 = p.tx * TW; p.y0 = p.ty * TH;
    p.base = (size_t)(blk / (unsigned)nty) * (size_t)H * W;
    return p;
}

// sx, sy: the tile's (TH + T - 1) x (TW + T - 1) operands, filled by every thread's own stores (this function starts with the barrier).
// Returns the thread's sum of the SSIM values of its TH * TW / NT windows that lie inside the image; ends behind a barrier, so hm is free.
template <int T>
__device__ __forceinline__ double tile_ssim(const double* sx, const double* sy, double (&hm)[5][TH + T - 1][TW], const double (&g)[T_MAX], double cov_norm, double c1,
                                            double c2, int x0, int y0, int H, int W)
{
    constexpr int HALO = T - 1, IW = TW + HALO, IH = TH + HALO;
    const int tid = threadIdx.x;
    __syncthreads();

    for (int i = tid; i < IH * TW; i += NT) {                     // horizontal pass: five maps, taps ascending
        const int r = i / TW, c = i % TW;
        const double* px = sx + r * IW + c;
        const double* py = sy + r * IW + c;
        double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const double x = px[k], y = py[k], gk = g[k];
            hx += gk * x; hy += gk * y; hxx += gk * (x * x); hyy += gk * (y * y); hxy += gk * (x * y);
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
            for (int k = 0; k < T; ++k) acc += g[k] * hm[q][oy + k][ox];
            m[q] = acc;
        }
        const double mux = m[0], muy = m[1];
        const double vx = cov_norm * (m[2] - mux * mux), vy = cov_norm * (m[3] - muy * muy), vxy = cov_norm * (m[4] - mux * muy);
        const double num = (2.0 * mux * muy + c1) * (2.0 * vxy + c2);
        const double den = (mux * mux + muy * muy + c1) * (vx + vy + c2);
        if (y0 + oy < H - HALO && x0 + ox < W - HALO) ss += num / den;
    }
    __syncthreads();
    return ss;
}

// the fixed tree over the 256 partial sums of each of V kinds: red[v * NT + tid] holds thread tid's value of kind v, red[v * NT] ends with the sum
template <int V>
__device__ __forceinline__ void tree_sum(double* red)
{
    const int tid = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int v = 0; v < V; ++v) red[v * NT + tid] += red[v * NT + tid + s];
        }
        __syncthreads();
    }
}

// tiles of one image (3 planes), 0 with the error set when the shape or the window is refused
inline long plan(const char* name, int B, int H, int W, int taps, int* ntx, int* nty)
{
    char msg[240];
    if (taps < T_MIN || taps > T_MAX || taps % 2 == 0) {
        snprintf(msg, sizeof msg, "%s: need an odd number of window taps, 3 <= taps <= 11, got %d", name, taps); set_last_error(msg); return 0;
    }
    if (B < 1 || H < taps || W < taps) {
        snprintf(msg, sizeof msg, "%s: need B >= 1 and H, W >= taps (H, W >= %d: one window), got B %d, %d x %d", name, taps, B, H, W); set_last_error(msg); return 0;
    }
    const long hw = (long)H * W;
    if (hw >= (1l << 31) / 3 || (long)B > ((1l << 31) - 1) / (3 * hw)) {
        snprintf(msg, sizeof msg, "%s: B * 3 * H * W must stay below 2^31, got B %d, %d x %d", name, B, H, W); set_last_error(msg); return 0;
    }
    const int halo = taps - 1;
    *ntx = (W - halo + TW - 1) / TW; *nty = (H - halo + TH - 1) / TH;
    return 3l * *ntx * *nty;
}

}  // namespace ssim
}  // namespace selftok
