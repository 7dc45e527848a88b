// Device image views (include/selftok_hip_ext.h): V outputs of S x S taken from packed uint8 HWC sources, each by a descriptor row
//   crop(x0, y0, bw, bh) -> resize to Rw x Rh [Pillow's 8-bit bilinear resample, each axis on its own] -> window (left, top, S, S) -> flip -> lut[u8]
// which is torchvision's five / ten-crop, resized_crop and hflip on a PIL image, bit for bit.  The arithmetic is that of image_io.hip (fp64 tap
// weights in Pillow's order, every operation rounded on its own; 22-bit coefficients; horizontal pass first, uint8 between the passes); the tap
// helpers are restated here rather than shared through a header because image_io.hip is also compiled on its own as a single file by its
// host stand-in test.  Four launches: plan (per-view check, the box rows its window reads, where they live between the passes), tables
// (one tap row per output index of the window, both axes), horizontal pass (those rows, the window's S columns) -> uint8 workspace,
// vertical pass + table lookup -> out, the flip being a reversed column index at the store.  A source named by several views is read in place.
#include "common.h"
#include "selftok_hip_ext.h"
#include <stdio.h>

#pragma clang fp contract(off)

namespace selftok {
namespace {

constexpr int PRECISION_BITS = 22;            // Pillow: 32 - 8 - 2
constexpr int HDR = 20;                       // ints per view header
constexpr int NV = 12;                        // longs per descriptor row
constexpr int MAX_S = 4096, MAX_SIDE = 65536;
enum { D_OFF, D_W, D_H, D_X0, D_Y0, D_BW, D_BH, D_RW, D_RH, D_LEFT, D_TOP, D_FLIP };
enum { H_VALID, H_W, H_X0, H_Y0, H_BW, H_BH, H_RW, H_RH, H_LEFT, H_TOP, H_FLIP, H_ROW0, H_NROWS, H_INTER_LO, H_INTER_HI, H_OFF_LO, H_OFF_HI };

// first input index and tap count of output index xx (Pillow's precompute_coeffs; `center` and 1 / filterscale come back for the weights)
__host__ __device__ inline void tap_bounds(int in, int out, int xx, double* center, double* ss, int* xmin, int* n)
{
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    const double c = (xx + 0.5) * scale;
    int lo = (int)(c - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(c + support + 0.5);
    if (hi > in) hi = in;
    *center = c;
    *ss = 1.0 / fs;
    *xmin = lo;
    *n = hi - lo;
}

__host__ __device__ inline int max_taps(int in, int out)          // Pillow's ksize: ceil(support) * 2 + 1
{
    if (in == out) return 1;
    const double scale = (double)in / (double)out;
    const double support = scale < 1.0 ? 1.0 : scale;
    int c = (int)support;
    if ((double)c < support) c++;
    return 2 * c + 1;
}

struct Geom { int row0, nrows, kh, kv; };
enum { G_OK, G_SIDE, G_BOX, G_RESIZED, G_WINDOW, G_FLIP, G_ROWS };

// the limits of one descriptor row (all but the byte range) and the box rows the window's S output rows read
__host__ __device__ inline int geometry(const long* d, int S, Geom* g)
{
    const long w = d[D_W], h = d[D_H], x0 = d[D_X0], y0 = d[D_Y0], bw = d[D_BW], bh = d[D_BH], rw = d[D_RW], rh = d[D_RH], left = d[D_LEFT], top = d[D_TOP];
    if (w < 1 || h < 1 || w > MAX_SIDE || h > MAX_SIDE) return G_SIDE;
    if (bw < 1 || bh < 1 || bw > w || bh > h || x0 < 0 || y0 < 0 || x0 > w - bw || y0 > h - bh) return G_BOX;
    if (rw < S || rh < S || rw >= (1l << 30) || rh >= (1l << 30)) return G_RESIZED;
    if (left < 0 || top < 0 || left > rw - S || top > rh - S) return G_WINDOW;
    if (d[D_FLIP] != 0 && d[D_FLIP] != 1) return G_FLIP;
    if (bh == rh) { g->row0 = (int)top; g->nrows = S; }
    else {
        double c, ss; int a0, n0, a1, n1;
        tap_bounds((int)bh, (int)rh, (int)top, &c, &ss, &a0, &n0);
        tap_bounds((int)bh, (int)rh, (int)top + S - 1, &c, &ss, &a1, &n1);
        g->row0 = a0; g->nrows = a1 + n1 - a0;
    }
    g->kh = max_taps((int)bw, (int)rw); g->kv = max_taps((int)bh, (int)rh);
    return (g->nrows >= 1 && g->row0 >= 0 && g->row0 + g->nrows <= bh) ? G_OK : G_ROWS;
}

__host__ __device__ inline bool bytes_ok(const long* d, size_t packed_bytes)      // after geometry(): w, h <= 65536, so 3 * w * h cannot overflow
{
    return d[D_OFF] >= 0 && (size_t)d[D_OFF] <= packed_bytes && (size_t)(3 * d[D_W] * d[D_H]) <= packed_bytes - (size_t)d[D_OFF];
}

__host__ __device__ inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct Layout { long htab, ksh, vtab, ksv; size_t inter, inter_bytes, total; int max_rows; };

bool plan_host(const long* t, int V, int S, Layout* L, const size_t* packed_bytes)
{
    static const char* const why[] = {"", "a source side outside 1 .. 65536", "a box that is empty or outside the source", "a resized side below S or >= 2^30",
                                      "a window outside the resized box", "a flip that is neither 0 nor 1", "no box row under its window"};
    char msg[256];
    if (!t || V < 1 || V > 65535 || S < 1 || S > MAX_S) { set_last_error("img_views: need a view table, 1 <= V <= 65535 and 1 <= S <= 4096"); return false; }
    int kh = 1, kv = 1, max_rows = 1;
    size_t inter = 0;
    for (int v = 0; v < V; ++v) {
        const long* d = t + (size_t)v * NV;
        Geom g;
        const int bad = geometry(d, S, &g);
        if (bad) {
            snprintf(msg, sizeof msg, "img_views: view %d has %s (source %ld x %ld, box %ld,%ld %ld x %ld -> %ld x %ld, window %ld,%ld, S %d, flip %ld)", v, why[bad],
                     d[D_W], d[D_H], d[D_X0], d[D_Y0], d[D_BW], d[D_BH], d[D_RW], d[D_RH], d[D_LEFT], d[D_TOP], S, d[D_FLIP]);
            set_last_error(msg); return false;
        }
        if (d[D_OFF] < 0 || (packed_bytes && !bytes_ok(d, *packed_bytes))) {
            snprintf(msg, sizeof msg, "img_views: the source of view %d (offset %ld, %ld x %ld x 3 bytes) reaches past the packed buffer", v, d[D_OFF], d[D_W], d[D_H]);
            set_last_error(msg); return false;
        }
        kh = g.kh > kh ? g.kh : kh; kv = g.kv > kv ? g.kv : kv; max_rows = g.nrows > max_rows ? g.nrows : max_rows;
        inter += align16((size_t)g.nrows * S * 3);
    }
    L->htab = (long)V * HDR; L->ksh = 2 + kh;
    L->vtab = L->htab + (long)V * S * L->ksh; L->ksv = 2 + kv;
    L->inter = align16(sizeof(int) * (size_t)(L->vtab + (long)V * S * L->ksv));
    L->inter_bytes = inter; L->total = L->inter + inter; L->max_rows = max_rows;
    return true;
}

struct Args {
    const unsigned char* packed; size_t packed_bytes; const long* views; int V, S;
    int* ws; long htab, ksh, vtab, ksv; unsigned char* inter; size_t inter_bytes; int max_rows;
};

__global__ void __launch_bounds__(256) views_plan_kernel(Args a)
{
    for (int v = threadIdx.x; v < a.V; v += 256) {
        int* hd = a.ws + (size_t)v * HDR;
        const long* d = a.views + (size_t)v * NV;
        Geom g;
        bool ok = geometry(d, a.S, &g) == G_OK && bytes_ok(d, a.packed_bytes);
        ok = ok && g.kh + 2 <= a.ksh && g.kv + 2 <= a.ksv && g.nrows <= a.max_rows;       // what the host sized the launch and the workspace for
        hd[H_VALID] = ok;
        if (!ok) { hd[H_NROWS] = 0; continue; }
        hd[H_W] = (int)d[D_W]; hd[H_X0] = (int)d[D_X0]; hd[H_Y0] = (int)d[D_Y0]; hd[H_BW] = (int)d[D_BW]; hd[H_BH] = (int)d[D_BH];
        hd[H_RW] = (int)d[D_RW]; hd[H_RH] = (int)d[D_RH]; hd[H_LEFT] = (int)d[D_LEFT]; hd[H_TOP] = (int)d[D_TOP]; hd[H_FLIP] = (int)d[D_FLIP];
        hd[H_ROW0] = g.row0; hd[H_NROWS] = g.nrows;
        hd[H_OFF_LO] = (int)(d[D_OFF] & 0xFFFFFFFFl); hd[H_OFF_HI] = (int)(d[D_OFF] >> 32);
    }
    __syncthreads();
    if (threadIdx.x == 0) {                     // where each view's rows between the passes live: a running sum over the views
        size_t at = 0;
        for (int v = 0; v < a.V; ++v) {
            int* hd = a.ws + (size_t)v * HDR;
            const size_t need = align16((size_t)hd[H_NROWS] * a.S * 3);
            if (at + need > a.inter_bytes) hd[H_VALID] = 0;
            hd[H_INTER_LO] = (int)(at & 0xFFFFFFFFu); hd[H_INTER_HI] = (int)(at >> 32);
            if (hd[H_VALID]) at += need;
        }
    }
}

__device__ __forceinline__ size_t hdr64(const int* hd, int lo) { return (size_t)(unsigned)hd[lo] | ((size_t)(unsigned)hd[lo + 1] << 32); }

// grid (V, 2): axis 0 = horizontal (output columns left .. left + S of the resized box), axis 1 = vertical.  One tap row per output index:
// [first box index, n, k...]
__global__ void __launch_bounds__(256) views_tables_kernel(Args a)
{
    const int v = blockIdx.x, axis = blockIdx.y;
    const int* hd = a.ws + (size_t)v * HDR;
    if (!hd[H_VALID]) return;
    const int in = axis ? hd[H_BH] : hd[H_BW], out = axis ? hd[H_RH] : hd[H_RW], first = axis ? hd[H_TOP] : hd[H_LEFT];
    const long ks = axis ? a.ksv : a.ksh;
    int* tab = a.ws + (axis ? a.vtab : a.htab) + (size_t)v * a.S * ks;
    const int lo_ok = axis ? hd[H_ROW0] : 0, hi_ok = axis ? hd[H_ROW0] + hd[H_NROWS] : in;
    for (int i = threadIdx.x; i < a.S; i += 256) {
        int* row = tab + (size_t)i * ks;
        const int xx = first + i;
        if (in == out) { row[0] = xx; row[1] = 1; row[2] = 1 << PRECISION_BITS; continue; }     // no pass along this axis: the identity tap
        double center, ss; int xmin, n;
        tap_bounds(in, out, xx, &center, &ss, &xmin, &n);
        if (n < 0 || n > ks - 2 || xmin < lo_ok || xmin + n > hi_ok) n = 0;                      // cannot happen (Pillow's own ksize bound); never read outside
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            double t = (x + xmin - center + 0.5) * ss;
            if (t < 0.0) t = -t;
            ww += t < 1.0 ? 1.0 - t : 0.0;
        }
        row[0] = xmin; row[1] = n;
        for (int x = 0; x < n; ++x) {
            double t = (x + xmin - center + 0.5) * ss;
            if (t < 0.0) t = -t;
            double wgt = t < 1.0 ? 1.0 - t : 0.0;
            if (ww != 0.0) wgt /= ww;
            row[2 + x] = wgt < 0.0 ? (int)(-0.5 + wgt * (double)(1 << PRECISION_BITS)) : (int)(0.5 + wgt * (double)(1 << PRECISION_BITS));
        }
    }
}

__device__ __forceinline__ int clip8(int v) { v >>= PRECISION_BITS; return v < 0 ? 0 : (v > 255 ? 255 : v); }

// grid (ceil(max_rows * S / 256), V): one thread = one (box row, window column) pixel, columns fastest
__global__ void __launch_bounds__(256) views_hpass_kernel(Args a)
{
    const int v = blockIdx.y;
    const int* hd = a.ws + (size_t)v * HDR;
    if (!hd[H_VALID]) return;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)hd[H_NROWS] * a.S) return;
    const int r = (int)(p / a.S), i = (int)(p % a.S);
    const int* row = a.ws + a.htab + ((size_t)v * a.S + i) * a.ksh;
    const int xmin = row[0], n = row[1];
    const unsigned char* src = a.packed + hdr64(hd, H_OFF_LO) + ((size_t)(hd[H_Y0] + hd[H_ROW0] + r) * hd[H_W] + hd[H_X0] + xmin) * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < n; ++x) {
        const int k = row[2 + x];
        s0 += src[3 * x] * k; s1 += src[3 * x + 1] * k; s2 += src[3 * x + 2] * k;
    }
    unsigned char* dst = a.inter + hdr64(hd, H_INTER_LO) + (size_t)p * 3;
    dst[0] = (unsigned char)clip8(s0); dst[1] = (unsigned char)clip8(s1); dst[2] = (unsigned char)clip8(s2);
}

// grid (ceil(S * S / 256), V): one thread = one window pixel, columns fastest; planar store through the 256-entry table, at the mirrored
// column when the view is flipped
template <typename T>
__global__ void __launch_bounds__(256) views_vpass_kernel(Args a, T* __restrict__ out, const T* __restrict__ lut)
{
    const int v = blockIdx.y;
    const int* hd = a.ws + (size_t)v * HDR;
    if (!hd[H_VALID]) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.S * a.S) return;
    const int i = p / a.S, j = p % a.S;
    const int* row = a.ws + a.vtab + ((size_t)v * a.S + i) * a.ksv;
    const int xmin = row[0], n = row[1];
    const size_t pitch = (size_t)a.S * 3;
    const unsigned char* src = a.inter + hdr64(hd, H_INTER_LO) + (size_t)(xmin - hd[H_ROW0]) * pitch + (size_t)j * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < n; ++x) {
        const int k = row[2 + x];
        s0 += src[0] * k; s1 += src[1] * k; s2 += src[2] * k;
        src += pitch;
    }
    const size_t plane = (size_t)a.S * a.S;
    T* o = out + (size_t)v * 3 * plane + (size_t)i * a.S + (hd[H_FLIP] ? a.S - 1 - j : j);
    o[0] = lut[clip8(s0)]; o[plane] = lut[clip8(s1)]; o[2 * plane] = lut[clip8(s2)];
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

size_t selftok_img_views_u8_workspace_bytes(const long* views_host, int V, int S)
{
    Layout L;
    return plan_host(views_host, V, S, &L, nullptr) ? L.total : 0;
}

int selftok_img_views_tables_layout(const long* views_host, int V, int S, long* layout4)
{
    Layout L;
    if (!layout4) { set_last_error("img_views_tables_layout: null output"); return SELFTOK_EINVAL; }
    if (!plan_host(views_host, V, S, &L, nullptr)) return SELFTOK_EINVAL;
    layout4[0] = L.htab; layout4[1] = L.ksh; layout4[2] = L.vtab; layout4[3] = L.ksv;
    return SELFTOK_OK;
}

int selftok_img_views_u8(const unsigned char* packed, size_t packed_bytes, const long* views_host, const long* views_dev, int V, int S, void* out, int out_bf16,
                         const void* lut, void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    if (!packed || !views_dev || !out || !lut || !workspace) { set_last_error("img_views: null pointer"); return SELFTOK_EINVAL; }
    Layout L;
    if (!plan_host(views_host, V, S, &L, &packed_bytes)) return SELFTOK_EINVAL;
    if (workspace_bytes < L.total) { set_last_error("img_views: workspace smaller than selftok_img_views_u8_workspace_bytes"); return SELFTOK_EINVAL; }
    if (((uintptr_t)workspace & 15) != 0) { set_last_error("img_views: workspace must be 16-byte aligned"); return SELFTOK_EINVAL; }
    Args a{packed, packed_bytes, views_dev, V, S, (int*)workspace, L.htab, L.ksh, L.vtab, L.ksv, (unsigned char*)workspace + L.inter, L.inter_bytes, L.max_rows};
    hipLaunchKernelGGL(views_plan_kernel, dim3(1), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(views_tables_kernel, dim3(V, 2), dim3(256), 0, stream, a);
    const long hblocks = ((long)L.max_rows * S + 255) / 256, vblocks = ((long)S * S + 255) / 256;
    hipLaunchKernelGGL(views_hpass_kernel, dim3((unsigned)hblocks, V), dim3(256), 0, stream, a);
    if (out_bf16) hipLaunchKernelGGL(views_vpass_kernel<unsigned short>, dim3((unsigned)vblocks, V), dim3(256), 0, stream, a, (unsigned short*)out, (const unsigned short*)lut);
    else hipLaunchKernelGGL(views_vpass_kernel<float>, dim3((unsigned)vblocks, V), dim3(256), 0, stream, a, (float*)out, (const float*)lut);
    return check_launch("img_views kernels");
}

}  // extern "C"
