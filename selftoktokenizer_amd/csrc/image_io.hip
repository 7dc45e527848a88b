// Device image I/O (include/selftok_hip_ext.h): the two ends of the reference's user script around the tokenizer.
//   in : uint8 HWC images of any sizes -> Resize(S) [Pillow's 8-bit bilinear resample, bit for bit] -> CenterCrop(S) -> lut[u8]
//   out: [B, 3, H, W] in [0, 1] -> uint8 [B, H, W, 3] with save_image's arithmetic in the tensor's own type
// The only floating-point part of the resample is the coefficient table: fp64, every operation rounded on its own (the build passes
// -ffp-contract=off; the pragma below says it again for this file), evaluated in Pillow's order (src/libImaging/Resample.c:
// precompute_coeffs, normalize_coeffs_8bpc).  The pixels are 32-bit integer sums of uint8 x 22-bit coefficients.
// Four launches: plan (per-image geometry + where its intermediate rows live), tables (one tap row per output index of the crop
// window, both axes), horizontal pass (only the input rows the crop window's rows touch, only its S columns) -> uint8 workspace,
// vertical pass + table lookup -> out.  Memory-bound and small (tens of MB per batch); the stage is bound by the host and the copy.
#include "common.h"
#include "selftok_hip_ext.h"
#include <stdio.h>

#pragma clang fp contract(off)

namespace selftok {
namespace {

constexpr int PRECISION_BITS = 22;            // Pillow: 32 - 8 - 2
constexpr int HDR = 16;                       // ints per image header
constexpr int MAX_S = 4096, MAX_SIDE = 65536;
enum { H_VALID, H_W, H_H, H_OW, H_OH, H_LEFT, H_TOP, H_ROW0, H_NROWS, H_PAD, H_INTER_LO, H_INTER_HI, H_OFF_LO, H_OFF_HI };

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

__host__ __device__ inline int crop_offset(int side, int S)       // int(round((side - S) / 2.0)), Python's round: half to even
{
    const int d = side - S, q = d >> 1;
    return (d & 1) ? q + (q & 1) : q;
}

struct Geom { int ow, oh, left, top, row0, nrows, kh, kv; };

// torchvision Resize(S) on a PIL image + CenterCrop(S): target size, crop origin, the input rows the crop window's rows read
__host__ __device__ inline bool geometry(long w, long h, int S, Geom* g)
{
    if (w < 1 || h < 1 || w > MAX_SIDE || h > MAX_SIDE) return false;
    long long ow, oh;
    if (w < h) { ow = S; oh = (long long)((double)((long long)S * h) / (double)w); }
    else       { oh = S; ow = (long long)((double)((long long)S * w) / (double)h); }
    if (ow < S || oh < S || ow >= (1ll << 30) || oh >= (1ll << 30)) return false;
    g->ow = (int)ow; g->oh = (int)oh;
    g->left = crop_offset(g->ow, S); g->top = crop_offset(g->oh, S);
    if ((int)h == g->oh) { g->row0 = g->top; g->nrows = S; }
    else {
        double c, ss; int x0, n0, x1, n1;
        tap_bounds((int)h, g->oh, g->top, &c, &ss, &x0, &n0);
        tap_bounds((int)h, g->oh, g->top + S - 1, &c, &ss, &x1, &n1);
        g->row0 = x0; g->nrows = x1 + n1 - x0;
    }
    g->kh = max_taps((int)w, g->ow); g->kv = max_taps((int)h, g->oh);
    return g->nrows >= 1 && g->row0 >= 0 && g->row0 + g->nrows <= h;
}

__host__ __device__ inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct Layout { long htab, ksh, vtab, ksv; size_t inter, inter_bytes, total; int max_rows; };

bool plan_host(const long* t, int B, int S, Layout* L, const size_t* packed_bytes)
{
    char msg[200];
    if (!t || B < 1 || S < 1 || S > MAX_S) { set_last_error("img_resize_crop_norm: need a table, B >= 1 and 1 <= S <= 4096"); return false; }
    int kh = 1, kv = 1, max_rows = 1;
    size_t inter = 0;
    for (int b = 0; b < B; ++b) {
        const long off = t[3 * b], w = t[3 * b + 1], h = t[3 * b + 2];
        Geom g;
        if (w < 1 || h < 1) { snprintf(msg, sizeof msg, "img_resize_crop_norm: image %d has a zero side (%ld x %ld)", b, w, h); set_last_error(msg); return false; }
        if (!geometry(w, h, S, &g)) { snprintf(msg, sizeof msg, "img_resize_crop_norm: image %d (%ld x %ld) is outside the limits (side <= 65536, resized side < 2^30)", b, w, h); set_last_error(msg); return false; }
        if (off < 0 || (packed_bytes && ((size_t)off > *packed_bytes || (size_t)(3 * w * h) > *packed_bytes - (size_t)off))) {
            snprintf(msg, sizeof msg, "img_resize_crop_norm: image %d (offset %ld, %ld x %ld x 3 bytes) reaches past the packed buffer", b, off, w, h); set_last_error(msg); return false;
        }
        kh = g.kh > kh ? g.kh : kh; kv = g.kv > kv ? g.kv : kv; max_rows = g.nrows > max_rows ? g.nrows : max_rows;
        inter += align16((size_t)g.nrows * S * 3);
    }
    L->htab = (long)B * HDR; L->ksh = 2 + kh;
    L->vtab = L->htab + (long)B * S * L->ksh; L->ksv = 2 + kv;
    L->inter = align16(sizeof(int) * (size_t)(L->vtab + (long)B * S * L->ksv));
    L->inter_bytes = inter; L->total = L->inter + inter; L->max_rows = max_rows;
    return true;
}

struct Args {
    const unsigned char* packed; size_t packed_bytes; const long* table; int B, S;
    int* ws; long htab, ksh, vtab, ksv; unsigned char* inter; size_t inter_bytes; int max_rows;
};

__global__ void __launch_bounds__(256) img_plan_kernel(Args a)
{
    for (int b = threadIdx.x; b < a.B; b += 256) {
        int* hd = a.ws + (size_t)b * HDR;
        const long off = a.table[3 * b], w = a.table[3 * b + 1], h = a.table[3 * b + 2];
        Geom g;
        bool ok = geometry(w, h, a.S, &g) && off >= 0 && (size_t)off <= a.packed_bytes && (size_t)(3 * w * h) <= a.packed_bytes - (size_t)off;
        ok = ok && g.kh + 2 <= a.ksh && g.kv + 2 <= a.ksv && g.nrows <= a.max_rows;       // what the host sized the launch and the workspace for
        hd[H_VALID] = ok;
        if (!ok) { hd[H_NROWS] = 0; continue; }
        hd[H_W] = (int)w; hd[H_H] = (int)h; hd[H_OW] = g.ow; hd[H_OH] = g.oh; hd[H_LEFT] = g.left; hd[H_TOP] = g.top; hd[H_ROW0] = g.row0; hd[H_NROWS] = g.nrows;
        hd[H_OFF_LO] = (int)(off & 0xFFFFFFFFl); hd[H_OFF_HI] = (int)(off >> 32);
    }
    __syncthreads();
    if (threadIdx.x == 0) {                     // where each image's rows between the passes live: a running sum, B is small
        size_t at = 0;
        for (int b = 0; b < a.B; ++b) {
            int* hd = a.ws + (size_t)b * HDR;
            const size_t need = align16((size_t)hd[H_NROWS] * a.S * 3);
            if (at + need > a.inter_bytes) hd[H_VALID] = 0;
            hd[H_INTER_LO] = (int)(at & 0xFFFFFFFFu); hd[H_INTER_HI] = (int)(at >> 32);
            if (hd[H_VALID]) at += need;
        }
    }
}

__device__ __forceinline__ size_t hdr64(const int* hd, int lo) { return (size_t)(unsigned)hd[lo] | ((size_t)(unsigned)hd[lo + 1] << 32); }

// grid (B, 2): axis 0 = horizontal (output columns left .. left + S), axis 1 = vertical.  One tap row per output index: [first, n, k...]
__global__ void __launch_bounds__(256) img_tables_kernel(Args a)
{
    const int b = blockIdx.x, axis = blockIdx.y;
    const int* hd = a.ws + (size_t)b * HDR;
    if (!hd[H_VALID]) return;
    const int in = axis ? hd[H_H] : hd[H_W], out = axis ? hd[H_OH] : hd[H_OW], first = axis ? hd[H_TOP] : hd[H_LEFT];
    const long ks = axis ? a.ksv : a.ksh;
    int* tab = a.ws + (axis ? a.vtab : a.htab) + (size_t)b * a.S * ks;
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
            double v = (x + xmin - center + 0.5) * ss;
            if (v < 0.0) v = -v;
            ww += v < 1.0 ? 1.0 - v : 0.0;
        }
        row[0] = xmin; row[1] = n;
        for (int x = 0; x < n; ++x) {
            double v = (x + xmin - center + 0.5) * ss;
            if (v < 0.0) v = -v;
            double wgt = v < 1.0 ? 1.0 - v : 0.0;
            if (ww != 0.0) wgt /= ww;
            row[2 + x] = wgt < 0.0 ? (int)(-0.5 + wgt * (double)(1 << PRECISION_BITS)) : (int)(0.5 + wgt * (double)(1 << PRECISION_BITS));
        }
    }
}

__device__ __forceinline__ int clip8(int v) { v >>= PRECISION_BITS; return v < 0 ? 0 : (v > 255 ? 255 : v); }

// grid (ceil(max_rows * S / 256), B): one thread = one (input row, crop column) pixel, columns fastest
__global__ void __launch_bounds__(256) img_hpass_kernel(Args a)
{
    const int b = blockIdx.y;
    const int* hd = a.ws + (size_t)b * HDR;
    if (!hd[H_VALID]) return;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)hd[H_NROWS] * a.S) return;
    const int r = (int)(p / a.S), i = (int)(p % a.S);
    const int* row = a.ws + a.htab + ((size_t)b * a.S + i) * a.ksh;
    const int xmin = row[0], n = row[1];
    const unsigned char* src = a.packed + hdr64(hd, H_OFF_LO) + ((size_t)(hd[H_ROW0] + r) * hd[H_W] + xmin) * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < n; ++x) {
        const int k = row[2 + x];
        s0 += src[3 * x] * k; s1 += src[3 * x + 1] * k; s2 += src[3 * x + 2] * k;
    }
    unsigned char* dst = a.inter + hdr64(hd, H_INTER_LO) + (size_t)p * 3;
    dst[0] = (unsigned char)clip8(s0); dst[1] = (unsigned char)clip8(s1); dst[2] = (unsigned char)clip8(s2);
}

// grid (ceil(S * S / 256), B): one thread = one output pixel, columns fastest; planar store through the 256-entry table
template <typename T>
__global__ void __launch_bounds__(256) img_vpass_kernel(Args a, T* __restrict__ out, const T* __restrict__ lut)
{
    const int b = blockIdx.y;
    const int* hd = a.ws + (size_t)b * HDR;
    if (!hd[H_VALID]) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.S * a.S) return;
    const int i = p / a.S, j = p % a.S;
    const int* row = a.ws + a.vtab + ((size_t)b * a.S + i) * a.ksv;
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
    T* o = out + (size_t)b * 3 * plane + p;
    o[0] = lut[clip8(s0)]; o[plane] = lut[clip8(s1)]; o[2 * plane] = lut[clip8(s2)];
}

__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ float round_bf16(float f)              // fp32 -> nearest bf16 (ties to even), as fp32; not for NaN
{
    unsigned u = __float_as_uint(f);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return __uint_as_float(u & 0xFFFF0000u);
}

template <bool BF16>
__device__ __forceinline__ unsigned char to_u8_one(float x)
{
    if (x != x) return 0;                                         // NaN: this project's choice
    float y = x * 255.0f;
    if (BF16) y = round_bf16(y);
    y = y + 0.5f;
    if (BF16) y = round_bf16(y);
    y = y < 0.0f ? 0.0f : (y > 255.0f ? 255.0f : y);
    return (unsigned char)(int)y;
}

template <bool BF16>
__global__ void __launch_bounds__(256) img_to_u8_kernel(const void* __restrict__ img, unsigned char* __restrict__ out, int B, int HW)
{
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)B * HW) return;
    const int b = (int)(p / HW), q = (int)(p % HW);
    const size_t base = (size_t)b * 3 * HW + q;
    unsigned char v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float x = BF16 ? bf16_to_f32(((const unsigned short*)img)[base + (size_t)c * HW]) : ((const float*)img)[base + (size_t)c * HW];
        v[c] = to_u8_one<BF16>(x);
    }
    unsigned char* o = out + (size_t)p * 3;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

size_t selftok_img_resize_crop_norm_u8_workspace_bytes(const long* table_host, int B, int S)
{
    Layout L;
    return plan_host(table_host, B, S, &L, nullptr) ? L.total : 0;
}

int selftok_img_resize_tables_layout(const long* table_host, int B, int S, long* layout4)
{
    Layout L;
    if (!layout4) { set_last_error("img_resize_tables_layout: null output"); return SELFTOK_EINVAL; }
    if (!plan_host(table_host, B, S, &L, nullptr)) return SELFTOK_EINVAL;
    layout4[0] = L.htab; layout4[1] = L.ksh; layout4[2] = L.vtab; layout4[3] = L.ksv;
    return SELFTOK_OK;
}

int selftok_img_resize_crop_norm_u8(const unsigned char* packed, size_t packed_bytes, const long* table_host, const long* table_dev, int B, int S, void* out,
                                    int out_bf16, const void* lut, void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    if (!packed || !table_dev || !out || !lut || !workspace) { set_last_error("img_resize_crop_norm: null pointer"); return SELFTOK_EINVAL; }
    if (B > 65535) { set_last_error("img_resize_crop_norm: B > 65535"); return SELFTOK_EINVAL; }
    Layout L;
    if (!plan_host(table_host, B, S, &L, &packed_bytes)) return SELFTOK_EINVAL;
    if (workspace_bytes < L.total) { set_last_error("img_resize_crop_norm: workspace smaller than selftok_img_resize_crop_norm_u8_workspace_bytes"); return SELFTOK_EINVAL; }
    if (((uintptr_t)workspace & 15) != 0) { set_last_error("img_resize_crop_norm: workspace must be 16-byte aligned"); return SELFTOK_EINVAL; }
    Args a{packed, packed_bytes, table_dev, B, S, (int*)workspace, L.htab, L.ksh, L.vtab, L.ksv, (unsigned char*)workspace + L.inter, L.inter_bytes, L.max_rows};
    hipLaunchKernelGGL(img_plan_kernel, dim3(1), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(img_tables_kernel, dim3(B, 2), dim3(256), 0, stream, a);
    const long hblocks = ((long)L.max_rows * S + 255) / 256, vblocks = ((long)S * S + 255) / 256;
    hipLaunchKernelGGL(img_hpass_kernel, dim3((unsigned)hblocks, B), dim3(256), 0, stream, a);
    if (out_bf16) hipLaunchKernelGGL(img_vpass_kernel<unsigned short>, dim3((unsigned)vblocks, B), dim3(256), 0, stream, a, (unsigned short*)out, (const unsigned short*)lut);
    else hipLaunchKernelGGL(img_vpass_kernel<float>, dim3((unsigned)vblocks, B), dim3(256), 0, stream, a, (float*)out, (const float*)lut);
    return check_launch("img_resize_crop_norm kernels");
}

int selftok_img_to_u8(const void* img, int in_bf16, unsigned char* out, int B, int H, int W, hipStream_t stream)
{
    if (!img || !out || B < 0 || H < 1 || W < 1 || (long)B * H * W >= (1l << 31)) { set_last_error("img_to_u8: bad argument (need B >= 0, H, W >= 1, B * H * W < 2^31)"); return SELFTOK_EINVAL; }
    if (B == 0) return SELFTOK_OK;
    const long n = (long)B * H * W;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (in_bf16) hipLaunchKernelGGL(img_to_u8_kernel<true>, dim3(blocks), dim3(256), 0, stream, img, out, B, H * W);
    else hipLaunchKernelGGL(img_to_u8_kernel<false>, dim3(blocks), dim3(256), 0, stream, img, out, B, H * W);
    return check_launch("img_to_u8_kernel");
}

}  // extern "C"
