// Device image input with a chosen Pillow filter (include/selftok_hip_ext.h): BILINEAR, BICUBIC or BOX, Pillow's own codes.
//   selftok_img_views_filter_u8   selftok_img_views_u8 (csrc/image_views.hip) with the filter as one more argument: the same [V, 12] rows, limits,
//                                 workspace layout and outputs, the tap rows as wide as the filter's support needs
//   selftok_img_resize_u8         Image.resize((ow, oh), filter) of whole uint8 HWC frames that live in one packed buffer, the results written
//                                 into that buffer: the BOX halvings of the ADM centre crop, a frame per row of six longs
// The arithmetic -- filter_weight, tap_row (precompute_coeffs + normalize_coeffs_8bpc), tap_sum3 and clip8 -- is image_resample_shared.h's, one text
// for every entry.  This file owns the row types, the whole-frame entry's workspace (per-frame tap rows and the uint8 rows between the passes, laid
// out by running sums that the device repeats on its own copy of the table) and its five small kernels.  Memory-bound and tiny next to the decode.
#include "common.h"
#include "selftok_hip_ext.h"
#include "image_resample_shared.h"
#include <stdio.h>
#include <algorithm>
#include <vector>

#pragma clang fp contract(off)

namespace selftok {
namespace {

struct FilterViewRow {                        // [V, 12]: the descriptor itself, as csrc/image_views.hip's
    static constexpr int COLS = NV, MAX_N = MAX_OUTPUTS;
    static constexpr const char* WHO = "img_views_filter";
    static constexpr const char* QUERY = "selftok_img_views_filter_u8_workspace_bytes";
    static constexpr const char* NEED = "img_views_filter: need a view table, 1 <= V <= 65535 and 1 <= S <= 4096";

    __host__ __device__ static void describe(const long* r, int, long* d)
    {
        for (int i = 0; i < NV; ++i) d[i] = r[i];
    }

    static void refuse(int v, int bad, const long* d, int S)
    {
        static const char* const why[] = {"", "a source side outside 1 .. 65536", "a box that is empty or outside the source", "a resized side below S or >= 2^30",
                                          "a window outside the resized box", "a flip that is neither 0 nor 1", "no box row under its window"};
        char msg[256];
        if (bad == G_BYTES) snprintf(msg, sizeof msg, "img_views_filter: the source of view %d (offset %ld, %ld x %ld x 3 bytes) reaches past the packed buffer", v, d[D_OFF], d[D_W], d[D_H]);
        else snprintf(msg, sizeof msg, "img_views_filter: view %d has %s (source %ld x %ld, box %ld,%ld %ld x %ld -> %ld x %ld, window %ld,%ld, S %d, flip %ld)", v, why[bad],
                      d[D_W], d[D_H], d[D_X0], d[D_Y0], d[D_BW], d[D_BH], d[D_RW], d[D_RH], d[D_LEFT], d[D_TOP], S, d[D_FLIP]);
        set_last_error(msg);
    }
};

// ---- whole frames: one row of six longs per frame ----
constexpr int RC = 6;
enum { R_SOFF, R_W, R_H, R_DOFF, R_OW, R_OH };
enum { Q_VALID, Q_W, Q_H, Q_OW, Q_OH, Q_KSH, Q_KSV, Q_HTAB_LO, Q_HTAB_HI, Q_VTAB_LO, Q_VTAB_HI, Q_INTER_LO, Q_INTER_HI, Q_SOFF_LO, Q_SOFF_HI, Q_DOFF_LO, Q_DOFF_HI };
enum { B_OK, B_SIDE, B_SRC, B_DST, B_OVERLAP };

struct Need { size_t htab, vtab, inter; int ksh, ksv; };       // ints, ints, bytes: what one frame takes of the workspace

// the limits of one row and what it needs; sides <= 65536, so no product below can overflow 64 bits
__host__ __device__ inline int frame_check(const long* r, size_t packed_bytes, int filter, Need* q)
{
    const long w = r[R_W], h = r[R_H], ow = r[R_OW], oh = r[R_OH];
    if (w < 1 || h < 1 || ow < 1 || oh < 1 || w > MAX_SIDE || h > MAX_SIDE || ow > MAX_SIDE || oh > MAX_SIDE) return B_SIDE;
    if (r[R_SOFF] < 0 || (size_t)r[R_SOFF] > packed_bytes || (size_t)(3 * w * h) > packed_bytes - (size_t)r[R_SOFF]) return B_SRC;
    if (r[R_DOFF] < 0 || (size_t)r[R_DOFF] > packed_bytes || (size_t)(3 * ow * oh) > packed_bytes - (size_t)r[R_DOFF]) return B_DST;
    q->ksh = 2 + max_taps((int)w, (int)ow, filter); q->ksv = 2 + max_taps((int)h, (int)oh, filter);
    q->htab = (size_t)ow * q->ksh; q->vtab = (size_t)oh * q->ksv;
    q->inter = align16((size_t)h * ow * 3);
    return B_OK;
}

__host__ __device__ inline bool overlaps(long a, long an, long b, long bn) { return a < b + bn && b < a + an; }

struct RLayout { size_t htab, htab_ints, vtab, vtab_ints, inter, inter_bytes, total; long max_h_px, max_v_px, max_o; };

void refuse_frame(int n, int bad, const long* r)
{
    static const char* const why[] = {"", "a side outside 1 .. 65536", "a source that reaches past the packed buffer", "a destination that reaches past the packed buffer",
                                      "a destination that overlaps a source or a destination of the same call"};
    char msg[256];
    snprintf(msg, sizeof msg, "img_resize: frame %d has %s (source offset %ld, %ld x %ld -> destination offset %ld, %ld x %ld)", n, why[bad], r[R_SOFF], r[R_W], r[R_H],
             r[R_DOFF], r[R_OW], r[R_OH]);
    set_last_error(msg);
}

// checks the host table and sizes the workspace; packed_bytes null (the query): offsets are only checked for their sign
bool rplan_host(const long* t, int N, int filter, RLayout* L, const size_t* packed_bytes)
{
    if (!filter_ok(filter)) return filter_refusal("img_resize", filter);
    if (!t || N < 1 || N > MAX_OUTPUTS) { set_last_error("img_resize: need a frame table and 1 <= N <= 65535"); return false; }
    const size_t limit = packed_bytes ? *packed_bytes : ~(size_t)0 >> 1;
    size_t hi = 0, vi = 0, ib = 0;
    long mh = 1, mv = 1, mo = 1;
    for (int n = 0; n < N; ++n) {
        const long* r = t + (size_t)n * RC;
        Need q;
        const int bad = frame_check(r, limit, filter, &q);
        if (bad) { refuse_frame(n, bad, r); return false; }
        hi += q.htab; vi += q.vtab; ib += q.inter;
        mh = std::max(mh, r[R_H] * r[R_OW]); mv = std::max(mv, r[R_OH] * r[R_OW]); mo = std::max(mo, std::max(r[R_OW], r[R_OH]));
    }
    // no destination may meet a source or another destination: sort the destinations, then every region looks up its neighbours
    std::vector<std::pair<long, int>> dst(N);
    for (int n = 0; n < N; ++n) dst[n] = {t[(size_t)n * RC + R_DOFF], n};
    std::sort(dst.begin(), dst.end());
    auto dbytes = [&](int n) { return 3 * t[(size_t)n * RC + R_OW] * t[(size_t)n * RC + R_OH]; };
    for (int i = 0; i + 1 < N; ++i)
        if (dst[i].first + dbytes(dst[i].second) > dst[i + 1].first) { refuse_frame(dst[i + 1].second, B_OVERLAP, t + (size_t)dst[i + 1].second * RC); return false; }
    for (int n = 0; n < N; ++n) {              // the destinations are disjoint and sorted: the last one that starts below the source's end is the only candidate
        const long* r = t + (size_t)n * RC;
        const long s0 = r[R_SOFF], s1 = s0 + 3 * r[R_W] * r[R_H];
        auto it = std::lower_bound(dst.begin(), dst.end(), std::make_pair(s1, -1));
        if (it != dst.begin()) {
            --it;
            if (it->first + dbytes(it->second) > s0) { refuse_frame(it->second, B_OVERLAP, t + (size_t)it->second * RC); return false; }
        }
    }
    L->htab = (size_t)N * HDR; L->htab_ints = hi;
    L->vtab = L->htab + hi; L->vtab_ints = vi;
    L->inter = align16(sizeof(int) * (L->vtab + vi)); L->inter_bytes = ib;
    L->total = L->inter + ib;
    L->max_h_px = mh; L->max_v_px = mv; L->max_o = mo;
    return true;
}

struct RArgs {
    unsigned char* packed; size_t packed_bytes; const long* table; int N, filter;
    int* ws; size_t htab, htab_ints, vtab, vtab_ints; unsigned char* inter; size_t inter_bytes; long max_h_px, max_v_px, max_o;
};

__device__ __forceinline__ void put64(int* hd, int lo, size_t v) { hd[lo] = (int)(v & 0xFFFFFFFFu); hd[lo + 1] = (int)(v >> 32); }

// grid ceil(N / 256): one thread = one row of the DEVICE table against the limits, the launch the host sized and every other row's regions
__global__ void __launch_bounds__(256) resize_check_kernel(RArgs a)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= a.N) return;
    int* hd = a.ws + (size_t)n * HDR;
    const long* r = a.table + (size_t)n * RC;
    Need q;
    bool ok = frame_check(r, a.packed_bytes, a.filter, &q) == B_OK;
    ok = ok && r[R_H] * r[R_OW] <= a.max_h_px && r[R_OH] * r[R_OW] <= a.max_v_px && r[R_OW] <= a.max_o && r[R_OH] <= a.max_o;
    if (ok) {
        const long d0 = r[R_DOFF], dn = 3 * r[R_OW] * r[R_OH];
        for (int m = 0; m < a.N && ok; ++m) {
            const long* o = a.table + (size_t)m * RC;
            if (o[R_W] < 1 || o[R_H] < 1 || o[R_OW] < 1 || o[R_OH] < 1 || o[R_W] > MAX_SIDE || o[R_H] > MAX_SIDE || o[R_OW] > MAX_SIDE || o[R_OH] > MAX_SIDE) continue;   // never runs
            if (overlaps(d0, dn, o[R_SOFF], 3 * o[R_W] * o[R_H])) ok = false;
            if (m != n && overlaps(d0, dn, o[R_DOFF], 3 * o[R_OW] * o[R_OH])) ok = false;
        }
    }
    hd[Q_VALID] = ok;
    if (!ok) return;
    hd[Q_W] = (int)r[R_W]; hd[Q_H] = (int)r[R_H]; hd[Q_OW] = (int)r[R_OW]; hd[Q_OH] = (int)r[R_OH]; hd[Q_KSH] = q.ksh; hd[Q_KSV] = q.ksv;
    put64(hd, Q_SOFF_LO, (size_t)r[R_SOFF]); put64(hd, Q_DOFF_LO, (size_t)r[R_DOFF]);
}

// one thread: where each valid frame's tap rows and rows between the passes live, running sums in table order; a frame that no longer fits
// what the host sized is skipped
__global__ void __launch_bounds__(64) resize_layout_kernel(RArgs a)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    size_t hi = 0, vi = 0, ib = 0;
    for (int n = 0; n < a.N; ++n) {
        int* hd = a.ws + (size_t)n * HDR;
        if (!hd[Q_VALID]) continue;
        const size_t nh = (size_t)hd[Q_OW] * hd[Q_KSH], nv = (size_t)hd[Q_OH] * hd[Q_KSV], nb = align16((size_t)hd[Q_H] * hd[Q_OW] * 3);
        if (hi + nh > a.htab_ints || vi + nv > a.vtab_ints || ib + nb > a.inter_bytes) { hd[Q_VALID] = 0; continue; }
        put64(hd, Q_HTAB_LO, a.htab + hi); put64(hd, Q_VTAB_LO, a.vtab + vi); put64(hd, Q_INTER_LO, ib);
        hi += nh; vi += nv; ib += nb;
    }
}

// grid (2 * ceil(max_o / 256), N): the first half of x = the ow horizontal tap rows of frame y, the second half = its oh vertical ones
__global__ void __launch_bounds__(256) resize_tables_kernel(RArgs a)
{
    const int* hd = a.ws + (size_t)blockIdx.y * HDR;
    if (!hd[Q_VALID]) return;
    const unsigned half = (unsigned)((a.max_o + 255) / 256);
    const int axis = blockIdx.x >= half;
    const int in = axis ? hd[Q_H] : hd[Q_W], out = axis ? hd[Q_OH] : hd[Q_OW], ks = axis ? hd[Q_KSV] : hd[Q_KSH];
    const long i = (long)(blockIdx.x - (axis ? half : 0u)) * 256 + threadIdx.x;
    if (i >= out) return;
    tap_row(in, out, (int)i, a.filter, ks, 0, in, a.ws + hdr64(hd, axis ? Q_VTAB_LO : Q_HTAB_LO) + (size_t)i * ks);
}

// grid (ceil(max_h_px / 256), N): one thread = one (source row, output column) pixel -> the uint8 rows between the passes, [H][ow][3]
__global__ void __launch_bounds__(256) resize_hpass_kernel(RArgs a)
{
    const int* hd = a.ws + (size_t)blockIdx.y * HDR;
    if (!hd[Q_VALID]) return;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const int ow = hd[Q_OW];
    if (p >= (long)hd[Q_H] * ow) return;
    const long r = p / ow; const int i = (int)(p % ow);
    const int* row = a.ws + hdr64(hd, Q_HTAB_LO) + (size_t)i * hd[Q_KSH];
    int s0, s1, s2;
    tap_sum3(a.packed + hdr64(hd, Q_SOFF_LO) + ((size_t)r * hd[Q_W] + row[0]) * 3, 3, row, s0, s1, s2);
    unsigned char* dst = a.inter + hdr64(hd, Q_INTER_LO) + (size_t)p * 3;
    dst[0] = (unsigned char)clip8(s0); dst[1] = (unsigned char)clip8(s1); dst[2] = (unsigned char)clip8(s2);
}

// grid (ceil(max_v_px / 256), N): one thread = one output pixel -> the frame's destination in `packed`, [oh][ow][3]
__global__ void __launch_bounds__(256) resize_vpass_kernel(RArgs a)
{
    const int* hd = a.ws + (size_t)blockIdx.y * HDR;
    if (!hd[Q_VALID]) return;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const int ow = hd[Q_OW];
    if (p >= (long)hd[Q_OH] * ow) return;
    const long i = p / ow; const int j = (int)(p % ow);
    const int* row = a.ws + hdr64(hd, Q_VTAB_LO) + (size_t)i * hd[Q_KSV];
    const size_t pitch = (size_t)ow * 3;
    int s0, s1, s2;
    tap_sum3(a.inter + hdr64(hd, Q_INTER_LO) + (size_t)row[0] * pitch + (size_t)j * 3, pitch, row, s0, s1, s2);
    unsigned char* dst = a.packed + hdr64(hd, Q_DOFF_LO) + (size_t)p * 3;
    dst[0] = (unsigned char)clip8(s0); dst[1] = (unsigned char)clip8(s1); dst[2] = (unsigned char)clip8(s2);
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

size_t selftok_img_views_filter_u8_workspace_bytes(const long* views_host, int V, int S, int filter)
{
    Layout L;
    return plan_host<FilterViewRow>(views_host, V, S, &L, nullptr, filter) ? L.total : 0;
}

int selftok_img_views_filter_tables_layout(const long* views_host, int V, int S, int filter, long* layout4)
{
    if (!layout4) { set_last_error("img_views_filter_tables_layout: null output"); return SELFTOK_EINVAL; }
    return tables_layout<FilterViewRow>(views_host, V, S, layout4, filter);
}

int selftok_img_views_filter_u8(const unsigned char* packed, size_t packed_bytes, const long* views_host, const long* views_dev, int V, int S, int filter, void* out,
                                int out_bf16, const void* lut, void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    return resample_run<FilterViewRow>(packed, packed_bytes, views_host, views_dev, V, S, out, out_bf16, lut, workspace, workspace_bytes, stream, filter);
}

size_t selftok_img_resize_u8_workspace_bytes(const long* frames_host, int N, int filter)
{
    RLayout L;
    return rplan_host(frames_host, N, filter, &L, nullptr) ? L.total : 0;
}

int selftok_img_resize_u8(unsigned char* packed, size_t packed_bytes, const long* frames_host, const long* frames_dev, int N, int filter, void* workspace,
                          size_t workspace_bytes, hipStream_t stream)
{
    if (!packed || !frames_dev || !workspace) return refuse_call("img_resize", "null pointer");
    RLayout L;
    if (!rplan_host(frames_host, N, filter, &L, &packed_bytes)) return SELFTOK_EINVAL;
    if (workspace_bytes < L.total) return refuse_call("img_resize", "workspace smaller than ", "selftok_img_resize_u8_workspace_bytes");
    if (((uintptr_t)workspace & 15) != 0) return refuse_call("img_resize", "workspace must be 16-byte aligned");
    RArgs a{packed, packed_bytes, frames_dev, N, filter, (int*)workspace, L.htab, L.htab_ints, L.vtab, L.vtab_ints, (unsigned char*)workspace + L.inter, L.inter_bytes,
            L.max_h_px, L.max_v_px, L.max_o};
    hipLaunchKernelGGL(resize_check_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(resize_layout_kernel, dim3(1), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(resize_tables_kernel, dim3(2 * (unsigned)((L.max_o + 255) / 256), N), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(resize_hpass_kernel, dim3((unsigned)((L.max_h_px + 255) / 256), N), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(resize_vpass_kernel, dim3((unsigned)((L.max_v_px + 255) / 256), N), dim3(256), 0, stream, a);
    return check_launch("img_resize kernels");
}

}  // extern "C"
