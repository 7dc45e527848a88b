// Pillow's 8-bit bilinear resample of a box of a packed uint8 HWC source, a window of the result, an optional flip and a 256-entry table, for N
// outputs of S x S: what csrc/image_io.hip (Resize(S) + CenterCrop(S), one [B, 3] row per image) and csrc/image_views.hip (one [V, 12] descriptor
// row per view) both run.  One definition each of the descriptor and its limits, the workspace layout, the four kernels and their launch, so that
// the arithmetic of record is one text.  The only floating-point part is the coefficient table: fp64, every operation rounded on its own (the
// build passes -ffp-contract=off; the pragma below says it again), evaluated in Pillow's order (src/libImaging/Resample.c: precompute_coeffs,
// normalize_coeffs_8bpc).  The pixels are 32-bit integer sums of uint8 x 22-bit coefficients, horizontal pass first, uint8 between the passes.
// Four launches: plan (per-output check, the box rows its window reads, where they live between the passes), tables (one tap row per output
// index of the window, both axes), horizontal pass (those rows, the window's S columns) -> uint8 workspace, vertical pass + table lookup -> out,
// the flip being a reversed column index at the store.  A source named by several rows is read in place.
//
// The filter is a run-time argument (Pillow's own codes: BILINEAR 2, BICUBIC 3, BOX 4), bilinear unless an entry says otherwise: `filter_support`
// and `filter_weight` are Pillow's bilinear_filter / bicubic_filter / box_filter, polynomials and comparisons only.  LANCZOS and HAMMING would
// need libm's sin / cos bit for bit and NEAREST is another code path of Pillow's: `filter_refusal` names them.  `tap_row` (one output index's
// taps) and `tap_sum3` (one pixel's three sums) are what every kernel here and the whole-frame resize of csrc/image_filters.hip evaluate.
//
// An entry names its table through a row type `Row`:
//   COLS                     longs per table row
//   MAX_N                    the most rows its host planner accepts (the launch itself takes 65535)
//   WHO, QUERY, NEED         the entry's name for the messages, its workspace query's name, the text that refuses a bad N or S
//   describe(row, S, d)      host and device: the row as the 12-long descriptor d (D_* below); must be safe on any row
//   refuse(n, bad, d, S)     host: set_last_error for row n, `bad` being the G_* code that refused it
#pragma once
#include "common.h"
#include <stdio.h>

#pragma clang fp contract(off)

namespace selftok {
namespace {                                   // per including unit: each entry's kernels are its own

constexpr int PRECISION_BITS = 22;            // Pillow: 32 - 8 - 2
constexpr int HDR = 20;                       // ints per output header
constexpr int NV = 12;                        // longs per descriptor
constexpr int MAX_S = 4096, MAX_SIDE = 65536, MAX_OUTPUTS = 65535;   // MAX_OUTPUTS: the grid's y extent
enum { F_NEAREST = 0, F_LANCZOS = 1, F_BILINEAR = 2, F_BICUBIC = 3, F_BOX = 4, F_HAMMING = 5 };                  // PIL.Image.Resampling
enum { D_OFF, D_W, D_H, D_X0, D_Y0, D_BW, D_BH, D_RW, D_RH, D_LEFT, D_TOP, D_FLIP };
enum { H_VALID, H_W, H_X0, H_Y0, H_BW, H_BH, H_RW, H_RH, H_LEFT, H_TOP, H_FLIP, H_ROW0, H_NROWS, H_INTER_LO, H_INTER_HI, H_OFF_LO, H_OFF_HI };

__host__ __device__ inline bool filter_ok(int filter) { return filter == F_BILINEAR || filter == F_BICUBIC || filter == F_BOX; }

__host__ __device__ inline double filter_support(int filter) { return filter == F_BICUBIC ? 2.0 : (filter == F_BOX ? 0.5 : 1.0); }

// Pillow's box_filter / bilinear_filter / bicubic_filter (a = -0.5) at the signed distance x: the box is open at -0.5 and closed at 0.5
__host__ __device__ inline double filter_weight(int filter, double x)
{
    if (filter == F_BOX) return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    if (x < 0.0) x = -x;
    if (filter == F_BICUBIC) {
        const double a = -0.5;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
    return x < 1.0 ? 1.0 - x : 0.0;
}

// first input index and tap count of output index xx (Pillow's precompute_coeffs; `center` and 1 / filterscale come back for the weights)
__host__ __device__ inline void tap_bounds(int in, int out, int xx, int filter, double* center, double* ss, int* xmin, int* n)
{
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = filter_support(filter) * fs;
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

__host__ __device__ inline int max_taps(int in, int out, int filter)          // Pillow's ksize: ceil(support) * 2 + 1
{
    if (in == out) return 1;
    const double scale = (double)in / (double)out;
    const double support = filter_support(filter) * (scale < 1.0 ? 1.0 : scale);
    int c = (int)support;
    if ((double)c < support) c++;
    return 2 * c + 1;
}

// the tap row of output index xx, [first input index, n, k...] in a row of `ks` ints: precompute_coeffs + normalize_coeffs_8bpc.  Taps outside
// lo_ok .. hi_ok would be read outside what the caller holds: the row is then empty
__host__ __device__ inline void tap_row(int in, int out, int xx, int filter, long ks, int lo_ok, int hi_ok, int* row)
{
    if (in == out) { row[0] = xx; row[1] = 1; row[2] = 1 << PRECISION_BITS; return; }                // no pass along this axis: the identity tap
    double center, ss; int xmin, n;
    tap_bounds(in, out, xx, filter, &center, &ss, &xmin, &n);
    if (n < 0 || n > ks - 2 || xmin < lo_ok || xmin + n > hi_ok) n = 0;                              // cannot happen (Pillow's own ksize bound); never read outside
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww += filter_weight(filter, (x + xmin - center + 0.5) * ss);
    row[0] = xmin; row[1] = n;
    for (int x = 0; x < n; ++x) {
        double wgt = filter_weight(filter, (x + xmin - center + 0.5) * ss);
        if (ww != 0.0) wgt /= ww;
        row[2 + x] = wgt < 0.0 ? (int)(-0.5 + wgt * (double)(1 << PRECISION_BITS)) : (int)(0.5 + wgt * (double)(1 << PRECISION_BITS));
    }
}

struct Geom { int row0, nrows, kh, kv; };
enum { G_OK, G_SIDE, G_BOX, G_RESIZED, G_WINDOW, G_FLIP, G_ROWS, G_BYTES };

// the limits of one descriptor (all but the byte range) and the box rows the window's S output rows read
__host__ __device__ inline int geometry(const long* d, int S, int filter, Geom* g)
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
        tap_bounds((int)bh, (int)rh, (int)top, filter, &c, &ss, &a0, &n0);
        tap_bounds((int)bh, (int)rh, (int)top + S - 1, filter, &c, &ss, &a1, &n1);
        g->row0 = a0; g->nrows = a1 + n1 - a0;
    }
    g->kh = max_taps((int)bw, (int)rw, filter); g->kv = max_taps((int)bh, (int)rh, filter);
    return (g->nrows >= 1 && g->row0 >= 0 && g->row0 + g->nrows <= bh) ? G_OK : G_ROWS;
}

__host__ __device__ inline bool bytes_ok(const long* d, size_t packed_bytes)      // after geometry(): w, h <= 65536, so 3 * w * h cannot overflow
{
    return d[D_OFF] >= 0 && (size_t)d[D_OFF] <= packed_bytes && (size_t)(3 * d[D_W] * d[D_H]) <= packed_bytes - (size_t)d[D_OFF];
}

__host__ __device__ inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// the workspace, in ints: [N][HDR] headers, [N][S][ksh] horizontal tap rows at htab, [N][S][ksv] vertical ones at vtab; then, from byte `inter`
// (16-aligned), each output's rows between the passes
struct Layout { long htab, ksh, vtab, ksv; size_t inter, inter_bytes, total; int max_rows; };

// checks the host table and sizes the workspace and the launch for it; `packed_bytes` null: the byte ranges are only checked for a negative offset
inline bool filter_refusal(const char* who, int filter);

template <typename Row>
bool plan_host(const long* t, int N, int S, Layout* L, const size_t* packed_bytes, int filter = F_BILINEAR)
{
    if (!filter_ok(filter)) return filter_refusal(Row::WHO, filter);
    if (!t || N < 1 || N > Row::MAX_N || S < 1 || S > MAX_S) { set_last_error(Row::NEED); return false; }
    int kh = 1, kv = 1, max_rows = 1;
    size_t inter = 0;
    for (int n = 0; n < N; ++n) {
        long d[NV];
        Row::describe(t + (size_t)n * Row::COLS, S, d);
        Geom g;
        int bad = geometry(d, S, filter, &g);
        if (!bad && (d[D_OFF] < 0 || (packed_bytes && !bytes_ok(d, *packed_bytes)))) bad = G_BYTES;
        if (bad) { Row::refuse(n, bad, d, S); return false; }
        kh = g.kh > kh ? g.kh : kh; kv = g.kv > kv ? g.kv : kv; max_rows = g.nrows > max_rows ? g.nrows : max_rows;
        inter += align16((size_t)g.nrows * S * 3);
    }
    L->htab = (long)N * HDR; L->ksh = 2 + kh;
    L->vtab = L->htab + (long)N * S * L->ksh; L->ksv = 2 + kv;
    L->inter = align16(sizeof(int) * (size_t)(L->vtab + (long)N * S * L->ksv));
    L->inter_bytes = inter; L->total = L->inter + inter; L->max_rows = max_rows;
    return true;
}

template <typename Row>
int tables_layout(const long* t, int N, int S, long* layout4, int filter = F_BILINEAR)
{
    Layout L;
    if (!plan_host<Row>(t, N, S, &L, nullptr, filter)) return SELFTOK_EINVAL;
    layout4[0] = L.htab; layout4[1] = L.ksh; layout4[2] = L.vtab; layout4[3] = L.ksv;
    return SELFTOK_OK;
}

struct Args {
    const unsigned char* packed; size_t packed_bytes; const long* table; int N, S;
    int* ws; long htab, ksh, vtab, ksv; unsigned char* inter; size_t inter_bytes; int max_rows; int filter;
};

// the device table is checked again, against the limits and against what the host sized: a row that disagrees is skipped (H_VALID = 0), the others run
template <typename Row>
__global__ void __launch_bounds__(256) resample_plan_kernel(Args a)
{
    for (int n = threadIdx.x; n < a.N; n += 256) {
        int* hd = a.ws + (size_t)n * HDR;
        long d[NV];
        Row::describe(a.table + (size_t)n * Row::COLS, a.S, d);
        Geom g;
        bool ok = geometry(d, a.S, a.filter, &g) == G_OK && bytes_ok(d, a.packed_bytes);
        ok = ok && g.kh + 2 <= a.ksh && g.kv + 2 <= a.ksv && g.nrows <= a.max_rows;       // what the host sized the launch and the workspace for
        hd[H_VALID] = ok;
        if (!ok) { hd[H_NROWS] = 0; continue; }
        hd[H_W] = (int)d[D_W]; hd[H_X0] = (int)d[D_X0]; hd[H_Y0] = (int)d[D_Y0]; hd[H_BW] = (int)d[D_BW]; hd[H_BH] = (int)d[D_BH];
        hd[H_RW] = (int)d[D_RW]; hd[H_RH] = (int)d[D_RH]; hd[H_LEFT] = (int)d[D_LEFT]; hd[H_TOP] = (int)d[D_TOP]; hd[H_FLIP] = (int)d[D_FLIP];
        hd[H_ROW0] = g.row0; hd[H_NROWS] = g.nrows;
        hd[H_OFF_LO] = (int)(d[D_OFF] & 0xFFFFFFFFl); hd[H_OFF_HI] = (int)(d[D_OFF] >> 32);
    }
    __syncthreads();
    if (threadIdx.x == 0) {                     // where each output's rows between the passes live: a running sum, N is small
        size_t at = 0;
        for (int n = 0; n < a.N; ++n) {
            int* hd = a.ws + (size_t)n * HDR;
            const size_t need = align16((size_t)hd[H_NROWS] * a.S * 3);
            if (at + need > a.inter_bytes) hd[H_VALID] = 0;
            hd[H_INTER_LO] = (int)(at & 0xFFFFFFFFu); hd[H_INTER_HI] = (int)(at >> 32);
            if (hd[H_VALID]) at += need;
        }
    }
}

__device__ __forceinline__ size_t hdr64(const int* hd, int lo) { return (size_t)(unsigned)hd[lo] | ((size_t)(unsigned)hd[lo + 1] << 32); }

// grid (N, 2): axis 0 = horizontal (output columns left .. left + S of the resized box), axis 1 = vertical.  One tap row per output index:
// [first box index, n, k...]
__global__ void __launch_bounds__(256) resample_tables_kernel(Args a)
{
    const int b = blockIdx.x, axis = blockIdx.y;
    const int* hd = a.ws + (size_t)b * HDR;
    if (!hd[H_VALID]) return;
    const int in = axis ? hd[H_BH] : hd[H_BW], out = axis ? hd[H_RH] : hd[H_RW], first = axis ? hd[H_TOP] : hd[H_LEFT];
    const long ks = axis ? a.ksv : a.ksh;
    int* tab = a.ws + (axis ? a.vtab : a.htab) + (size_t)b * a.S * ks;
    const int lo_ok = axis ? hd[H_ROW0] : 0, hi_ok = axis ? hd[H_ROW0] + hd[H_NROWS] : in;
    for (int i = threadIdx.x; i < a.S; i += 256) tap_row(in, out, first + i, a.filter, ks, lo_ok, hi_ok, tab + (size_t)i * ks);
}

__device__ __forceinline__ int clip8(int v) { v >>= PRECISION_BITS; return v < 0 ? 0 : (v > 255 ? 255 : v); }

// one pixel: (2^21 + sum of u8 x coefficient) of the three channels over the taps of `row`, the inputs `stride` bytes apart
__device__ __forceinline__ void tap_sum3(const unsigned char* src, size_t stride, const int* row, int& s0, int& s1, int& s2)
{
    const int n = row[1];
    s0 = s1 = s2 = 1 << (PRECISION_BITS - 1);
    for (int x = 0; x < n; ++x) {
        const int k = row[2 + x];
        s0 += src[0] * k; s1 += src[1] * k; s2 += src[2] * k;
        src += stride;
    }
}

// grid (ceil(max_rows * S / 256), N): one thread = one (box row, window column) pixel, columns fastest
__global__ void __launch_bounds__(256) resample_hpass_kernel(Args a)
{
    const int b = blockIdx.y;
    const int* hd = a.ws + (size_t)b * HDR;
    if (!hd[H_VALID]) return;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)hd[H_NROWS] * a.S) return;
    const int r = (int)(p / a.S), i = (int)(p % a.S);
    const int* row = a.ws + a.htab + ((size_t)b * a.S + i) * a.ksh;
    int s0, s1, s2;
    tap_sum3(a.packed + hdr64(hd, H_OFF_LO) + ((size_t)(hd[H_Y0] + hd[H_ROW0] + r) * hd[H_W] + hd[H_X0] + row[0]) * 3, 3, row, s0, s1, s2);
    unsigned char* dst = a.inter + hdr64(hd, H_INTER_LO) + (size_t)p * 3;
    dst[0] = (unsigned char)clip8(s0); dst[1] = (unsigned char)clip8(s1); dst[2] = (unsigned char)clip8(s2);
}

// grid (ceil(S * S / 256), N): one thread = one window pixel, columns fastest; planar store through the 256-entry table, at the mirrored
// column when the output is flipped
template <typename T>
__global__ void __launch_bounds__(256) resample_vpass_kernel(Args a, T* __restrict__ out, const T* __restrict__ lut)
{
    const int b = blockIdx.y;
    const int* hd = a.ws + (size_t)b * HDR;
    if (!hd[H_VALID]) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.S * a.S) return;
    const int i = p / a.S, j = p % a.S;
    const int* row = a.ws + a.vtab + ((size_t)b * a.S + i) * a.ksv;
    const size_t pitch = (size_t)a.S * 3;
    int s0, s1, s2;
    tap_sum3(a.inter + hdr64(hd, H_INTER_LO) + (size_t)(row[0] - hd[H_ROW0]) * pitch + (size_t)j * 3, pitch, row, s0, s1, s2);
    const size_t plane = (size_t)a.S * a.S;
    T* o = out + (size_t)b * 3 * plane + (size_t)i * a.S + (hd[H_FLIP] ? a.S - 1 - j : j);
    o[0] = lut[clip8(s0)]; o[plane] = lut[clip8(s1)]; o[2 * plane] = lut[clip8(s2)];
}

inline int refuse_call(const char* who, const char* what, const char* more = "")
{
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s%s", who, what, more);
    set_last_error(msg);
    return SELFTOK_EINVAL;
}

// why a filter code is not served; false, for plan_host
inline bool filter_refusal(const char* who, int filter)
{
    const char* name = filter == F_LANCZOS ? "LANCZOS" : filter == F_HAMMING ? "HAMMING" : filter == F_NEAREST ? "NEAREST" : "an unknown code";
    char msg[256];
    snprintf(msg, sizeof msg, "%s: filter %d (%s) is not served: %s; BILINEAR (2), BICUBIC (3) and BOX (4) are", who, filter, name,
             filter == F_LANCZOS || filter == F_HAMMING ? "its weights need libm's sin / cos bit for bit, which the device does not promise"
             : filter == F_NEAREST ? "Pillow does not resample it through its coefficient tables" : "Pillow has no such filter");
    set_last_error(msg);
    return false;
}

// the whole entry: pointers, the host table, the workspace, then the four launches on `stream`
template <typename Row>
int resample_run(const unsigned char* packed, size_t packed_bytes, const long* table_host, const long* table_dev, int N, int S, void* out, int out_bf16,
                 const void* lut, void* workspace, size_t workspace_bytes, hipStream_t stream, int filter = F_BILINEAR)
{
    if (!packed || !table_dev || !out || !lut || !workspace) return refuse_call(Row::WHO, "null pointer");
    Layout L;
    if (!plan_host<Row>(table_host, N, S, &L, &packed_bytes, filter)) return SELFTOK_EINVAL;
    if (N > MAX_OUTPUTS) return refuse_call(Row::WHO, "B > 65535");                               // only a Row whose MAX_N is larger gets here
    if (workspace_bytes < L.total) return refuse_call(Row::WHO, "workspace smaller than ", Row::QUERY);
    if (((uintptr_t)workspace & 15) != 0) return refuse_call(Row::WHO, "workspace must be 16-byte aligned");
    Args a{packed, packed_bytes, table_dev, N, S, (int*)workspace, L.htab, L.ksh, L.vtab, L.ksv, (unsigned char*)workspace + L.inter, L.inter_bytes, L.max_rows, filter};
    hipLaunchKernelGGL(resample_plan_kernel<Row>, dim3(1), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(resample_tables_kernel, dim3(N, 2), dim3(256), 0, stream, a);
    const long hblocks = ((long)L.max_rows * S + 255) / 256, vblocks = ((long)S * S + 255) / 256;
    hipLaunchKernelGGL(resample_hpass_kernel, dim3((unsigned)hblocks, N), dim3(256), 0, stream, a);
    if (out_bf16) hipLaunchKernelGGL(resample_vpass_kernel<unsigned short>, dim3((unsigned)vblocks, N), dim3(256), 0, stream, a, (unsigned short*)out, (const unsigned short*)lut);
    else hipLaunchKernelGGL(resample_vpass_kernel<float>, dim3((unsigned)vblocks, N), dim3(256), 0, stream, a, (float*)out, (const float*)lut);
    char what[64];
    snprintf(what, sizeof what, "%s kernels", Row::WHO);
    return check_launch(what);
}

}  // namespace
}  // namespace selftok
