// Token statistics on [N, K] matrices of code ids (include/selftok_hip_ext.h; selftoktokenizer_amd/tokenstats.py is the host side;
// tests/token_stats_cases.py restates every entry in numpy).  Integer arithmetic throughout, one fp64 entropy.
//
//   tok_count_kernel     one thread per id, flat over n_rows * K (256 ids per workgroup): counts[k * C + id] += 1 with a plain global atomic; an id outside
//                        [0, C) adds 1 to bad[0] and touches nothing else.  No LDS histogram: the callers that matter pass 64 rows per call.
//   tok_pool_kernel      pooled[c] = the uint64 sum of counts[k][c] over k ascending, one thread per code.
//   tok_census_kernel    one workgroup of 256 threads per output row (K positions, then the pooled counts).  Pass 1, integers: n, used, max_count.  Pass 2, fp64:
//                        thread t owns the codes t, t + 256, t + 512, .. and adds their terms from +0.0 in that order (a zero count adds nothing); the 64 lanes of a
//                        wave merge by the butterfly v + shfl_xor(v, o), o = 32 .. 1; the four waves add as ((w0 + w1) + w2) + w3.  No atomics: the same bits every run.
//                        H = 0.0 - sum p ln p, H_ref = 0.0 - sum p ln(p + 1e-10), p = (double)count / (double)n.
//   tok_to_u16_kernel    one thread per id: dense uint16 out, 0 and bad[0] += 1 for an id outside [0, 65535].
//   tok_agree_rows_kernel one wave per row: n_diff, first_diff (K if none), last_diff (-1 if none) over [k_lo, k_hi).
//   tok_agree_pos_kernel one thread per position and tile of 256 rows: the tile's matches counted in a register, one atomic per (tile, position).
//   tok_nearest_kernel   the compute-bound one.  256 threads; a workgroup owns a strip of 64 query rows and walks the 64-row reference tiles of its split.  Per
//                        tile, chunks of 64 positions of both sides are staged in LDS as 32-bit words (two ids each; a position outside [k_lo, k_hi) is staged as 0
//                        on BOTH sides, so it never differs).  Thread (tq, tr) = (tid % 16, tid / 16) holds the 4 x 4 pairs of queries tq + 16 i against references
//                        tr + 16 j and counts DIFFERING positions two at a time in packed 16-bit lanes: d = q - r (v_pk_sub_u16), min(d, 1) (v_pk_min_u16),
//                        acc += (v_pk_add_u16) -- three vector instructions per two comparisons, operands from ds_read_b128 (row stride 36 words: the 16 distinct
//                        query rows of a wave cover the 64 banks once).  match = (k_hi - k_lo) - differing.  A candidate is the 64-bit key
//                        (match + 1) << 32 | ~index, the best the LARGEST key: most matches, then lowest index; 0 = none.  References past the end, and the
//                        query's own index when asked, are masked BY INDEX.  Keys merge over tr by shfl_xor 16 / 32, over waves through LDS, and one key per
//                        (split, query) goes to the workspace; tok_nearest_finalize_kernel takes the maximum over the splits.  Integer maxima: no split changes a bit.
// No inline assembly, no scratch, no state.
#include "common.h"
#include "selftok_hip_ext.h"
#include <stdio.h>

namespace selftok {
namespace {

typedef unsigned long long u64;
typedef unsigned short u16;
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256;
constexpr long LIM = 1l << 31;

// ---- count -------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long load_id(const void* ids, int id_bytes, size_t off)
{
    if (id_bytes == 2) return (long long)((const u16*)ids)[off];
    if (id_bytes == 4) return (long long)((const int*)ids)[off];
    return ((const long long*)ids)[off];
}

__global__ void __launch_bounds__(NT) tok_count_kernel(const void* __restrict__ ids, int id_bytes, long total, int K, int C, long row_stride, long elem_stride,
                                                       unsigned* __restrict__ counts, unsigned* __restrict__ bad)
{
    const long e = (long)blockIdx.x * NT + threadIdx.x;
    if (e >= total) return;
    const long r = e / K;
    const int k = (int)(e - r * K);
    const long long id = load_id(ids, id_bytes, (size_t)(r * row_stride + k * elem_stride));
    if (id >= 0 && id < (long long)C) atomicAdd(counts + (size_t)k * C + (size_t)id, 1u);
    else atomicAdd(bad, 1u);
}

__global__ void __launch_bounds__(NT) tok_to_u16_kernel(const void* __restrict__ ids, int id_bytes, long total, int K, long row_stride, long elem_stride,
                                                        u16* __restrict__ out, unsigned* __restrict__ bad)
{
    const long e = (long)blockIdx.x * NT + threadIdx.x;
    if (e >= total) return;
    const long r = e / K;
    const int k = (int)(e - r * K);
    const long long id = load_id(ids, id_bytes, (size_t)(r * row_stride + k * elem_stride));
    const bool ok = id >= 0 && id <= 65535;
    out[e] = ok ? (u16)id : (u16)0;
    if (!ok) atomicAdd(bad, 1u);
}

// ---- census ------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) tok_pool_kernel(const unsigned* __restrict__ counts, u64* __restrict__ pooled, int K, int C)
{
    const int c = blockIdx.x * NT + threadIdx.x;
    if (c >= C) return;
    u64 s = 0;
    for (int k = 0; k < K; ++k) s += counts[(size_t)k * C + c];
    pooled[c] = s;
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int o)
{
    const unsigned lo = __shfl_xor((unsigned)v, o, WAVE), hi = __shfl_xor((unsigned)(v >> 32), o, WAVE);
    return ((u64)hi << 32) | lo;
}

__global__ void __launch_bounds__(NT) tok_census_kernel(const unsigned* __restrict__ counts, const u64* __restrict__ pooled, double* __restrict__ out, int K, int C)
{
    __shared__ u64 sn[NT / WAVE], su[NT / WAVE], sm[NT / WAVE];
    __shared__ double sh[NT / WAVE], sr[NT / WAVE];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool pool = row == K;
    const unsigned* cr = counts + (size_t)(pool ? 0 : row) * C;
    u64 n = 0, used = 0, mx = 0;
    for (int c = tid; c < C; c += NT) {
        const u64 v = pool ? pooled[c] : (u64)cr[c];
        n += v; used += v > 0 ? 1 : 0; mx = v > mx ? v : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n += shfl_xor_u64(n, o); used += shfl_xor_u64(used, o);
        const u64 m2 = shfl_xor_u64(mx, o); mx = m2 > mx ? m2 : mx;
    }
    if (lane == 0) { sn[wave] = n; su[wave] = used; sm[wave] = mx; }
    __syncthreads();
    n = sn[0] + sn[1] + sn[2] + sn[3];
    used = su[0] + su[1] + su[2] + su[3];
    mx = sm[0];
#pragma unroll
    for (int w = 1; w < NT / WAVE; ++w) mx = sm[w] > mx ? sm[w] : mx;

    double h = 0.0, hr = 0.0;
    if (n > 0) {
        const double dn = (double)n;
        for (int c = tid; c < C; c += NT) {
            const u64 v = pool ? pooled[c] : (u64)cr[c];
            if (v > 0) {
                const double p = (double)v / dn;
                h = h + p * log(p);
                hr = hr + p * log(p + 1e-10);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { h = h + __shfl_xor(h, o, WAVE); hr = hr + __shfl_xor(hr, o, WAVE); }
    if (lane == 0) { sh[wave] = h; sr[wave] = hr; }
    __syncthreads();
    if (tid == 0) {
        double* o = out + (size_t)row * 5;
        o[0] = (double)n; o[1] = (double)used;
        o[2] = 0.0 - (((sh[0] + sh[1]) + sh[2]) + sh[3]);
        o[3] = 0.0 - (((sr[0] + sr[1]) + sr[2]) + sr[3]);
        o[4] = (double)mx;
    }
}

// ---- agreement ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) tok_agree_rows_kernel(const u16* __restrict__ a, const u16* __restrict__ b, int n_rows, int K, int k_lo, int k_hi,
                                                            int* __restrict__ n_diff, int* __restrict__ first_diff, int* __restrict__ last_diff)
{
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * (NT / WAVE) + (threadIdx.x >> 6);
    if (r >= n_rows) return;                                       // the whole wave leaves together
    const u16* pa = a + (size_t)r * K;
    const u16* pb = b + (size_t)r * K;
    int nd = 0, first = K, last = -1;
    for (int k = k_lo + lane; k < k_hi; k += WAVE) {
        if (pa[k] != pb[k]) { nd += 1; first = k < first ? k : first; last = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nd += __shfl_xor(nd, o, WAVE);
        first = min(first, __shfl_xor(first, o, WAVE));
        last = max(last, __shfl_xor(last, o, WAVE));
    }
    if (lane == 0) { n_diff[r] = nd; first_diff[r] = first; last_diff[r] = last; }
}

// grid (ceil((k_hi - k_lo) / 256), ceil(n_rows / 256))
__global__ void __launch_bounds__(NT) tok_agree_pos_kernel(const u16* __restrict__ a, const u16* __restrict__ b, int n_rows, int K, int k_lo, int k_hi,
                                                           unsigned* __restrict__ match_pos)
{
    const int k = k_lo + blockIdx.x * NT + threadIdx.x;
    if (k >= k_hi) return;
    const long r0 = (long)blockIdx.y * NT;
    const long r1 = r0 + NT < n_rows ? r0 + NT : n_rows;
    unsigned m = 0;
    for (long r = r0; r < r1; ++r) m += a[(size_t)r * K + k] == b[(size_t)r * K + k] ? 1u : 0u;
    if (m) atomicAdd(match_pos + k, m);
}

// ---- nearest sequence --------------------------------------------------------------------------------------------------------------------------
constexpr int TN_ROWS = 64;                                       // query rows per strip, reference rows per tile
constexpr int TN_KC = 64;                                         // positions per staged chunk
constexpr int TN_W = TN_KC / 2;                                   // ... as 32-bit words
constexpr int TN_STRIDE = TN_W + 4;                               // 36: rows 16-byte aligned, 16 consecutive rows on 64 distinct banks under ds_read_b128
constexpr int TN_MAX_SPLIT = 64;
constexpr int TN_MAX_K = 65535;                                   // a packed 16-bit counter never wraps

// 64 rows x 32 words; thread t stages words t % 32 of rows t / 32 + 8 i.  Word w of the chunk holds positions kc + 2 w, kc + 2 w + 1.
template <bool ALIGNED>
__device__ __forceinline__ void tn_stage(unsigned* __restrict__ dst, const u16* __restrict__ src, long row0, long n_rows, int K, int kc, int k_lo, int k_hi)
{
    const int w = threadIdx.x & 31, rr = threadIdx.x >> 5;
    const int k = kc + 2 * w;
    const bool in0 = k >= k_lo && k < k_hi, in1 = k + 1 >= k_lo && k + 1 < k_hi;
#pragma unroll
    for (int i = 0; i < TN_ROWS / 8; ++i) {
        const int rl = rr + 8 * i;
        const long row = row0 + rl;
        unsigned v = 0;
        if (row < n_rows) {
            const u16* p = src + (size_t)row * K + k;
            if (ALIGNED) {                                        // K even, chunk origin even, base 4-byte aligned: one word, the out-of-range half cleared
                if (in0 || in1) { v = *(const unsigned*)p; if (!in1) v &= 0xFFFFu; if (!in0) v &= 0xFFFF0000u; }
            } else {
                if (in0) v = p[0];
                if (in1) v |= (unsigned)p[1] << 16;
            }
        }
        dst[rl * TN_STRIDE + w] = v;
    }
}

__device__ __forceinline__ u16x2 as_u16x2(unsigned v) { union { unsigned u; u16x2 h; } c; c.u = v; return c.h; }

template <bool ALIGNED>
__global__ void __launch_bounds__(NT) tok_nearest_kernel(const u16* __restrict__ q, int M, const u16* __restrict__ ref, int N, int K, int k_lo, int k_hi,
                                                         long self_off, int tiles_per_split, unsigned ones, u64* __restrict__ keys)
{
    __shared__ __attribute__((aligned(16))) unsigned Qs[TN_ROWS * TN_STRIDE];
    __shared__ __attribute__((aligned(16))) unsigned Rs[TN_ROWS * TN_STRIDE];
    __shared__ u64 wbest[NT / WAVE][TN_ROWS];
    const int tid = threadIdx.x, tq = tid & 15, tr = tid >> 4;
    const long q0 = (long)blockIdx.x * TN_ROWS;
    const int ntiles = (N + TN_ROWS - 1) / TN_ROWS;
    const int t_first = blockIdx.y * tiles_per_split;
    const int t_last = min(t_first + tiles_per_split, ntiles);
    const int span = k_hi - k_lo;
    const int kc0 = k_lo & ~1;                                    // chunk origins stay even

    const u16x2 one = as_u16x2(ones);                              // 0x00010001 from the host: a literal 1 is folded into compare / select / permute, six instructions for three
    u64 best[4] = {0, 0, 0, 0};
    for (int t = t_first; t < t_last; ++t) {
        const long r0 = (long)t * TN_ROWS;
        u16x2 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (u16x2)(0);
        for (int kc = kc0; kc < k_hi; kc += TN_KC) {
            __syncthreads();                                      // the previous chunk has been read
            tn_stage<ALIGNED>(Qs, q, q0, M, K, kc, k_lo, k_hi);
            tn_stage<ALIGNED>(Rs, ref, r0, N, K, kc, k_lo, k_hi);
            __syncthreads();
#pragma unroll
            for (int w = 0; w < TN_W; w += 4) {
                u32x4 qa[4], ra[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) qa[i] = *(const u32x4*)(Qs + (tq + 16 * i) * TN_STRIDE + w);
#pragma unroll
                for (int j = 0; j < 4; ++j) ra[j] = *(const u32x4*)(Rs + (tr + 16 * j) * TN_STRIDE + w);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const u16x2 d = as_u16x2(qa[i][e]) - as_u16x2(ra[j][e]);
                            acc[i][j] += __builtin_elementwise_min(d, one);
                        }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long qi = q0 + tq + 16 * i + self_off;          // self_off < 0: nothing is skipped (no index is negative)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long cand = r0 + tr + 16 * j;
                const int diff = (int)acc[i][j].x + (int)acc[i][j].y;
                const bool ok = cand < N && !(self_off >= 0 && cand == qi);
                const u64 key = ok ? (((u64)(unsigned)(span - diff + 1) << 32) | (u64)(~(unsigned)cand)) : 0ull;
                best[i] = key > best[i] ? key : best[i];
            }
        }
    }
    // over tr: lanes tq + 16 * (tr % 4) of a wave, then the four waves
    const int wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        u64 k = best[i];
        u64 o = shfl_xor_u64(k, 16); k = o > k ? o : k;
        o = shfl_xor_u64(k, 32); k = o > k ? o : k;
        if ((tid & 63) < 16) wbest[wave][tq + 16 * i] = k;
    }
    __syncthreads();
    if (tid < TN_ROWS && q0 + tid < M) {
        u64 k = wbest[0][tid];
#pragma unroll
        for (int w = 1; w < NT / WAVE; ++w) k = wbest[w][tid] > k ? wbest[w][tid] : k;
        keys[(size_t)blockIdx.y * M + q0 + tid] = k;
    }
}

__global__ void __launch_bounds__(NT) tok_nearest_finalize_kernel(const u64* __restrict__ keys, int* __restrict__ best_match, int* __restrict__ best_idx, int M, int parts)
{
    const int r = blockIdx.x * NT + threadIdx.x;
    if (r >= M) return;
    u64 k = 0;
    for (int p = 0; p < parts; ++p) {
        const u64 v = keys[(size_t)p * M + r];
        k = v > k ? v : k;
    }
    best_match[r] = k == 0 ? -1 : (int)(unsigned)(k >> 32) - 1;
    best_idx[r] = k == 0 ? 0 : (int)~(unsigned)k;
}

bool ids_ok(const char* who, int id_bytes, long n_rows, int K, long row_stride, long elem_stride)
{
    char msg[256];
    if (id_bytes != 2 && id_bytes != 4 && id_bytes != 8) {
        snprintf(msg, sizeof msg, "%s: id_bytes must be 2 (uint16), 4 (int32) or 8 (int64), got %d", who, id_bytes);
        set_last_error(msg); return false;
    }
    if (n_rows < 0 || K <= 0 || row_stride < 0 || elem_stride < 0 || (n_rows > 0 && n_rows > (LIM - 1) / K)) {
        snprintf(msg, sizeof msg, "%s: need n_rows >= 0, K >= 1, n_rows * K below 2^31 and strides >= 0, got n_rows %ld, K %d, strides %ld / %ld", who, n_rows, K,
                 row_stride, elem_stride);
        set_last_error(msg); return false;
    }
    return true;
}

bool range_ok(const char* who, int K, int k_lo, int k_hi)
{
    char msg[256];
    if (K <= 0 || K > TN_MAX_K || k_lo < 0 || k_lo > k_hi || k_hi > K) {
        snprintf(msg, sizeof msg, "%s: need 1 <= K <= %d and 0 <= k_lo <= k_hi <= K, got K %d, k_lo %d, k_hi %d", who, TN_MAX_K, K, k_lo, k_hi);
        set_last_error(msg); return false;
    }
    return true;
}

int nearest_max_parts(int N)
{
    const int ntiles = (N + TN_ROWS - 1) / TN_ROWS;
    return ntiles < 1 ? 1 : (ntiles < TN_MAX_SPLIT ? ntiles : TN_MAX_SPLIT);
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

int selftok_token_count(const void* ids, int id_bytes, long n_rows, int K, int C, long row_stride, long elem_stride, unsigned* counts, unsigned* bad,
                        hipStream_t stream)
{
    if (!ids_ok("token_count", id_bytes, n_rows, K, row_stride, elem_stride)) return SELFTOK_EINVAL;
    if (C <= 0 || (long)K * C >= LIM) { set_last_error("token_count: need C >= 1 and K * C below 2^31"); return SELFTOK_EINVAL; }
    if (!counts || !bad || (n_rows > 0 && !ids)) { set_last_error("token_count: null pointer"); return SELFTOK_EINVAL; }
    if (((uintptr_t)ids % (uintptr_t)id_bytes) != 0 || ((uintptr_t)counts & 3) != 0 || ((uintptr_t)bad & 3) != 0) {
        set_last_error("token_count: ids must be aligned to id_bytes, counts and bad to 4 bytes"); return SELFTOK_EINVAL;
    }
    if (n_rows == 0) return SELFTOK_OK;
    const long total = n_rows * K;
    hipLaunchKernelGGL(tok_count_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, stream, ids, id_bytes, total, K, C, row_stride, elem_stride, counts, bad);
    return check_launch("token_count kernel");
}

size_t selftok_token_census_workspace_bytes(int K, int C)
{
    if (K <= 0 || C <= 0 || (long)K * C >= LIM) { set_last_error("token_census: need K >= 1, C >= 1 and K * C below 2^31"); return 0; }
    return (size_t)C * sizeof(u64);
}

int selftok_token_census(const unsigned* counts, int K, int C, double* out, void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    const size_t need = selftok_token_census_workspace_bytes(K, C);
    if (!need) return SELFTOK_EINVAL;
    if (!counts || !out || !workspace) { set_last_error("token_census: null pointer"); return SELFTOK_EINVAL; }
    if (workspace_bytes < need) { set_last_error("token_census: workspace smaller than selftok_token_census_workspace_bytes"); return SELFTOK_EINVAL; }
    if (((uintptr_t)counts & 3) != 0 || ((uintptr_t)out & 7) != 0 || ((uintptr_t)workspace & 7) != 0) {
        set_last_error("token_census: counts must be 4-byte aligned, out and workspace 8-byte aligned"); return SELFTOK_EINVAL;
    }
    hipLaunchKernelGGL(tok_pool_kernel, dim3((unsigned)((C + NT - 1) / NT)), dim3(NT), 0, stream, counts, (u64*)workspace, K, C);
    hipLaunchKernelGGL(tok_census_kernel, dim3((unsigned)(K + 1)), dim3(NT), 0, stream, counts, (const u64*)workspace, out, K, C);
    return check_launch("token_census kernels");
}

int selftok_token_to_u16(const void* ids, int id_bytes, long n_rows, int K, long row_stride, long elem_stride, unsigned short* out, unsigned* bad,
                         hipStream_t stream)
{
    if (!ids_ok("token_to_u16", id_bytes, n_rows, K, row_stride, elem_stride)) return SELFTOK_EINVAL;
    if (!bad || (n_rows > 0 && (!ids || !out))) { set_last_error("token_to_u16: null pointer"); return SELFTOK_EINVAL; }
    if (((uintptr_t)ids % (uintptr_t)id_bytes) != 0 || ((uintptr_t)out & 1) != 0 || ((uintptr_t)bad & 3) != 0) {
        set_last_error("token_to_u16: ids must be aligned to id_bytes, out to 2 bytes, bad to 4"); return SELFTOK_EINVAL;
    }
    if (n_rows == 0) return SELFTOK_OK;
    const long total = n_rows * K;
    hipLaunchKernelGGL(tok_to_u16_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, stream, ids, id_bytes, total, K, row_stride, elem_stride, out, bad);
    return check_launch("token_to_u16 kernel");
}

int selftok_token_agree(const unsigned short* a, const unsigned short* b, int n_rows, int K, int k_lo, int k_hi, unsigned* match_pos, int* n_diff,
                        int* first_diff, int* last_diff, hipStream_t stream)
{
    if (!range_ok("token_agree", K, k_lo, k_hi)) return SELFTOK_EINVAL;
    if (n_rows < 0 || n_rows > 256 * 65535 || (n_rows > 0 && n_rows > (LIM - 1) / K)) {
        set_last_error("token_agree: need 0 <= n_rows <= 256 * 65535 and n_rows * K below 2^31"); return SELFTOK_EINVAL;
    }
    if (!match_pos || (n_rows > 0 && (!a || !b || !n_diff || !first_diff || !last_diff))) { set_last_error("token_agree: null pointer"); return SELFTOK_EINVAL; }
    if (((uintptr_t)a & 1) != 0 || ((uintptr_t)b & 1) != 0 || ((uintptr_t)match_pos & 3) != 0 || ((uintptr_t)n_diff & 3) != 0 || ((uintptr_t)first_diff & 3) != 0 ||
        ((uintptr_t)last_diff & 3) != 0) {
        set_last_error("token_agree: a and b must be 2-byte aligned, the outputs 4-byte aligned"); return SELFTOK_EINVAL;
    }
    if (n_rows == 0) return SELFTOK_OK;
    hipLaunchKernelGGL(tok_agree_rows_kernel, dim3((unsigned)((n_rows + NT / WAVE - 1) / (NT / WAVE))), dim3(NT), 0, stream, a, b, n_rows, K, k_lo, k_hi, n_diff,
                       first_diff, last_diff);
    if (k_hi > k_lo)
        hipLaunchKernelGGL(tok_agree_pos_kernel, dim3((unsigned)((k_hi - k_lo + NT - 1) / NT), (unsigned)((n_rows + NT - 1) / NT)), dim3(NT), 0, stream, a, b, n_rows,
                           K, k_lo, k_hi, match_pos);
    return check_launch("token_agree kernels");
}

size_t selftok_token_nearest_workspace_bytes(int M, int N)
{
    if (M < 0 || N < 0 || N > (int)(LIM - 1 - TN_ROWS)) { set_last_error("token_nearest: need M >= 0 queries and 0 <= N < 2^31 - 64 reference rows"); return 0; }
    return (size_t)nearest_max_parts(N) * (size_t)(M > 0 ? M : 1) * sizeof(u64);
}

int selftok_token_nearest(const unsigned short* q, int M, const unsigned short* ref, int N, int K, int k_lo, int k_hi, int exclude_self, int split, int* best_match,
                          int* best_idx, void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    const size_t need = selftok_token_nearest_workspace_bytes(M, N);
    if (!need) return SELFTOK_EINVAL;
    if (!range_ok("token_nearest", K, k_lo, k_hi)) return SELFTOK_EINVAL;
    if (exclude_self < 0 || split < 0) { set_last_error("token_nearest: exclude_self and split must be >= 0 (split 0 = automatic)"); return SELFTOK_EINVAL; }
    if (M > (LIM - 1) / K || (N > 0 && N > (LIM - 1) / K)) { set_last_error("token_nearest: need M * K and N * K below 2^31"); return SELFTOK_EINVAL; }
    if (M == 0) return SELFTOK_OK;
    if (!q || (N > 0 && !ref) || !best_match || !best_idx || !workspace) { set_last_error("token_nearest: null pointer"); return SELFTOK_EINVAL; }
    if (workspace_bytes < need) { set_last_error("token_nearest: workspace smaller than selftok_token_nearest_workspace_bytes"); return SELFTOK_EINVAL; }
    if (((uintptr_t)q & 1) != 0 || ((uintptr_t)ref & 1) != 0 || ((uintptr_t)workspace & 7) != 0 || ((uintptr_t)best_match & 3) != 0 || ((uintptr_t)best_idx & 3) != 0) {
        set_last_error("token_nearest: q and ref must be 2-byte aligned, best_match and best_idx 4-byte aligned, workspace 8-byte aligned"); return SELFTOK_EINVAL;
    }
    u64* keys = (u64*)workspace;
    int parts = 0;
    if (N > 0) {
        const int ntiles = (N + TN_ROWS - 1) / TN_ROWS, strips = (M + TN_ROWS - 1) / TN_ROWS;
        const int max_split = nearest_max_parts(N);
        int s = 1;                                                // splits until the grid holds about four workgroups per compute unit, every split four tiles deep
        while ((long)strips * s < 1024 && s * 2 <= max_split && ntiles / (s * 2) >= 4) s *= 2;
        if (split > 0) s = split < max_split ? split : max_split;
        const int tps = (ntiles + s - 1) / s;
        parts = (ntiles + tps - 1) / tps;                         // every split holds at least one tile
        const bool aligned = (K & 1) == 0 && ((uintptr_t)q & 3) == 0 && ((uintptr_t)ref & 3) == 0;
        const long self_off = exclude_self > 0 ? (long)(exclude_self - 1) : -1;
        const dim3 grid((unsigned)strips, (unsigned)parts);
        if (aligned) hipLaunchKernelGGL(tok_nearest_kernel<true>, grid, dim3(NT), 0, stream, q, M, ref, N, K, k_lo, k_hi, self_off, tps, 0x00010001u, keys);
        else hipLaunchKernelGGL(tok_nearest_kernel<false>, grid, dim3(NT), 0, stream, q, M, ref, N, K, k_lo, k_hi, self_off, tps, 0x00010001u, keys);
    }
    hipLaunchKernelGGL(tok_nearest_finalize_kernel, dim3((unsigned)((M + NT - 1) / NT)), dim3(NT), 0, stream, (const u64*)keys, best_match, best_idx, M, parts);
    return check_launch("token_nearest kernels");
}

}  // extern "C"
