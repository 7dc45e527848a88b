// Density / coverage, nearest neighbours and the Kernel Inception Distance on pool3 features (include/selftok_hip_ext.h;
// selftoktokenizer_amd/genmetrics.py states the definitions, GEN_METRICS_DEFINITION; tests/gen_metrics_kdc_cases.py restates them in numpy fp64).
//
// The pair arithmetic is csrc/gen_metrics_shared.h's and nothing else: gm::row_norm, the k-ascending chain of gm::tile_dots, gm::pair_d2.  This file has no
// matrix instruction, fused multiply-add, atomic or inline assembly of its own; the bits of d2(u, v) and of a dot product are the ones selftok_knn_radius_f32
// and selftok_manifold_member_f32 produce, a function of the two rows alone.
//
// Count / nearest (Naeem et al. 2020 need a COUNT of balls per query and a NEAREST distance per row; the membership entry keeps neither):
//   gm_count_nn_kernel: the launch geometry of gm_pairs_kernel -- 256 threads, one workgroup = a strip of 128 lane-side query rows against a contiguous run of
//     128-candidate tiles (grid: strips x column splits, the parent's split rule).  Epilogue per lane and row:
//       count  an int32 count of d2 <= r2[candidate] (false against NaN), skipped when there are no radii;
//       key    the running minimum of (bits of d2 << 32) | candidate as an unsigned 64-bit integer over the non-NaN distances: d2 is clamped at +0, non-negative
//              floats order as unsigned integers, so the minimum is the smallest distance and, on equal bits, the lowest candidate index; 2^64 - 1 = none.
//     Candidates past the end of the set are staged as zeros and masked BY INDEX: a zero row has a finite d2 that would win a minimum and count inside a big ball.
//     The two lane halves merge through the cross-lane network; parts go to workspace[part][row], part = 2 * split + the wave's candidate half.
//   gm_count_nn_finalize_kernel adds the counts and takes the minimum of the keys, both in integer arithmetic: every split gives the same bits.
//     No key: nn_d2 = NaN, nn_idx = -1.
//
// KID sums (Binkowski et al. 2018; k(u, v) = (u.v / D + 1)^3):
//   kid_tile_kernel: one workgroup per (subset s, which of XX / YY / XY, 128 x 128 tile): gm::tile_dots on the subset's m contiguous rows, then every IN-RANGE
//     element c becomes t = (double)c / (double)D + 1.0, (t * t) * t in fp64.  In range: row < m and column < m BY INDEX, and position row != column for XX / YY
//     (a zero-filled row would contribute (0 + 1)^3 = 1 per pair if masked by value).  Summation order:
//       lane   from +0.0 over its 64 accumulator registers in the order ci, ri, r ascending (a masked element adds nothing);
//       wave   the butterfly v = v + shfl_xor(v, o), o = 32, 16, .., 1 (commutative: every lane holds the same bits);
//       group  waves 0, 1, 2, 3 in that order through LDS;
//     one fp64 partial per tile into workspace[(s * 3 + which) * T * T + tile], T = ceil(m / 128), tile = row tile * T + column tile.
//   kid_finalize_kernel: sums[s][which] = the T * T partials added from +0.0 in ascending tile order.
//   The launch shape is a function of (S, m, D) alone: a subset's three sums depend on its own 2 m rows and on nothing else.
// No atomics, no state, no scratch: the outputs are functions of the inputs alone.
#include "common.h"

#pragma clang fp contract(off)

#include "gen_metrics_shared.h"
#include "selftok_hip_ext.h"
#include <stdio.h>

namespace selftok {
namespace {

using gm::BT; using gm::KT; using gm::LDS_STRIDE; using gm::NT; using gm::f32x16;

typedef unsigned long long u64;
constexpr u64 KEY_NONE = ~0ull;
constexpr int GM_MAX_SPLIT = 64;
constexpr long LIM = 1l << 31;
constexpr int KID_MAX_M = 1 << 22;                                // T * T tiles stay below 2^31
constexpr int KID_MAX_S = 65535;                                  // a grid dimension

// one row per thread
__global__ void __launch_bounds__(NT) kdc_norm_kernel(const float* __restrict__ x, float* __restrict__ norm, int N, int D)
{
    const int r = blockIdx.x * NT + threadIdx.x;
    if (r < N) norm[r] = gm::row_norm(x + (size_t)r * D, D);
}

struct CountArgs {
    const float* rows; const float* rnorm; int NR;                // lane side: the queries
    const float* cands; const float* cnorm; const float* cr2; int NC;      // register side: the set and its radii
    int D, tiles_per_split;
    u64* keys;                                                    // [parts][NR]
    int* counts;                                                  // [parts][NR]
};

template <bool COUNT>
__global__ void __launch_bounds__(NT) gm_count_nn_kernel(CountArgs a)
{
    __shared__ __attribute__((aligned(16))) float Rs[KT * LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) float Cs[KT * LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) float cn[BT];
    __shared__ __attribute__((aligned(16))) float cr[BT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fk = lane >> 5;
    const int rm = (wave & 1) * 64, cm = (wave >> 1) * 64;
    const long r0 = (long)blockIdx.x * BT;
    const int ntiles = (a.NC + BT - 1) / BT;
    const int t_first = blockIdx.y * a.tiles_per_split;
    const int t_last = min(t_first + a.tiles_per_split, ntiles);

    float rn[2];
#pragma unroll
    for (int ri = 0; ri < 2; ++ri) {
        const long r = r0 + rm + 32 * ri + fr;
        rn[ri] = r < a.NR ? a.rnorm[r] : 0.0f;
    }
    u64 best[2] = {KEY_NONE, KEY_NONE};
    int cnt[2] = {0, 0};

    for (int t = t_first; t < t_last; ++t) {
        const long c0 = (long)t * BT;
        __syncthreads();                                          // the previous tile's epilogue has read cn / cr
        if (tid < BT) {
            const long c = c0 + tid;
            cn[tid] = c < a.NC ? a.cnorm[c] : 0.0f;
            if (COUNT) cr[tid] = c < a.NC ? a.cr2[c] : 0.0f;
        }
        f32x16 acc[2][2];
        gm::tile_dots(a.rows, r0, a.NR, a.cands, c0, a.NC, a.D, Rs, Cs, acc);      // its barriers publish cn / cr
        const bool ragged = c0 + BT > a.NC;
#pragma unroll
        for (int ci = 0; ci < 2; ++ci) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int cl = cm + 32 * ci + 8 * q + 4 * fk;                       // candidates cl .. cl + 3 = accumulator registers 4 q .. 4 q + 3
                const float4 n4 = *(const float4*)(cn + cl);
                const float nn[4] = {n4.x, n4.y, n4.z, n4.w};
                float rr[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (COUNT) { const float4 r4 = *(const float4*)(cr + cl); rr[0] = r4.x; rr[1] = r4.y; rr[2] = r4.z; rr[3] = r4.w; }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const long cand = c0 + cl + j;
                    const bool ok = !ragged || cand < a.NC;                         // by index, never by value
#pragma unroll
                    for (int ri = 0; ri < 2; ++ri) {
                        const float d = gm::pair_d2(rn[ri], nn[j], acc[ci][ri][4 * q + j]);
                        const u64 key = (ok && d == d) ? (((u64)__float_as_uint(d) << 32) | (u64)(unsigned)cand) : KEY_NONE;
                        best[ri] = key < best[ri] ? key : best[ri];
                        if (COUNT) cnt[ri] += (ok && d <= rr[j]) ? 1 : 0;
                    }
                }
            }
        }
    }

    const int part = blockIdx.y * 2 + (wave >> 1);
#pragma unroll
    for (int ri = 0; ri < 2; ++ri) {
        const long r = r0 + rm + 32 * ri + fr;
        const unsigned olo = __shfl_xor((unsigned)best[ri], 32, WAVE), ohi = __shfl_xor((unsigned)(best[ri] >> 32), 32, WAVE);
        const u64 other = ((u64)ohi << 32) | olo;
        const u64 k = other < best[ri] ? other : best[ri];
        const int c = COUNT ? cnt[ri] + __shfl_xor(cnt[ri], 32, WAVE) : 0;
        if (fk == 0 && r < a.NR) {
            a.keys[(size_t)part * a.NR + r] = k;
            if (COUNT) a.counts[(size_t)part * a.NR + r] = c;
        }
    }
}

__global__ void __launch_bounds__(NT) gm_count_nn_finalize_kernel(const u64* __restrict__ keys, const int* __restrict__ counts, int* __restrict__ count,
                                                                  float* __restrict__ nn_d2, int* __restrict__ nn_idx, int M, int parts)
{
    const int r = blockIdx.x * NT + threadIdx.x;
    if (r >= M) return;
    u64 k = KEY_NONE;
    int c = 0;
    for (int p = 0; p < parts; ++p) {
        const u64 v = keys[(size_t)p * M + r];
        k = v < k ? v : k;
        if (count) c += counts[(size_t)p * M + r];
    }
    if (count) count[r] = c;
    nn_d2[r] = k == KEY_NONE ? __uint_as_float(0x7FC00000u) : __uint_as_float((unsigned)(k >> 32));
    nn_idx[r] = k == KEY_NONE ? -1 : (int)(unsigned)k;
}

// grid (T * T, 3, S)
__global__ void __launch_bounds__(NT) kid_tile_kernel(const float* __restrict__ xs, const float* __restrict__ ys, double* __restrict__ ws, int m, int D, int T)
{
    __shared__ __attribute__((aligned(16))) float Rs[KT * LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) float Cs[KT * LDS_STRIDE];
    __shared__ double wsum[NT / WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fk = lane >> 5;
    const int rm = (wave & 1) * 64, cm = (wave >> 1) * 64;
    const int which = blockIdx.y, s = blockIdx.z;
    const int tr = blockIdx.x / T, tc = blockIdx.x - tr * T;
    const long r0 = (long)tr * BT, c0 = (long)tc * BT;
    const size_t base = (size_t)s * m * D;
    const float* R = (which == 1 ? ys : xs) + base;
    const float* Cm = (which == 0 ? xs : ys) + base;

    f32x16 acc[2][2];
    gm::tile_dots(R, r0, m, Cm, c0, m, D, Rs, Cs, acc);
    const double dd = (double)D;
    double sum = 0.0;
#pragma unroll
    for (int ci = 0; ci < 2; ++ci)
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long row = r0 + rm + 32 * ri + fr, col = c0 + cm + 32 * ci + gm::acc_row(r, fk);
                const bool in = row < m && col < m && !(which < 2 && row == col);
                const double t = (double)acc[ci][ri][r] / dd + 1.0;
                const double k = (t * t) * t;
                sum = in ? sum + k : sum;
            }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum = sum + __shfl_xor(sum, o, WAVE);
    if (lane == 0) wsum[wave] = sum;
    __syncthreads();
    if (tid == 0) ws[((size_t)s * 3 + which) * T * T + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one thread per (subset, which)
__global__ void __launch_bounds__(NT) kid_finalize_kernel(const double* __restrict__ ws, double* __restrict__ sums, int n, long tiles)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const double* p = ws + (size_t)i * tiles;
    double v = 0.0;
    for (long t = 0; t < tiles; ++t) v = v + p[t];
    sums[i] = v;
}

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// the rule of gm_pairs_kernel's launches: column splits until the grid holds about four workgroups per compute unit, every split at least four tiles deep
int pick_split(int row_strips, int ntiles, int override_split)
{
    const int max_split = ntiles < GM_MAX_SPLIT ? ntiles : GM_MAX_SPLIT;
    int split = 1;
    while ((long)row_strips * split < 1024 && split * 2 <= max_split && ntiles / (split * 2) >= 4) split *= 2;
    if (override_split > 0) split = override_split < max_split ? override_split : max_split;
    return split;
}

bool rows_ok(const char* who, long n_rows, long n_cands, int D)
{
    char msg[256];
    if (D < 16 || D > 2048 || D % 16 != 0 || n_rows >= LIM / D || n_cands >= LIM / D) {
        snprintf(msg, sizeof msg, "%s: need D a multiple of 16 in 16 .. 2048 and rows * D below 2^31, got %ld and %ld rows, D %d", who, n_rows, n_cands, D);
        set_last_error(msg); return false;
    }
    return true;
}

bool kid_ok(int S, int m, int D)
{
    char msg[256];
    if (S < 1 || S > KID_MAX_S || m < 2 || m > KID_MAX_M) {
        snprintf(msg, sizeof msg, "kid_sums: need 1 <= S <= %d subsets of 2 <= m <= %d rows, got S %d, m %d", KID_MAX_S, KID_MAX_M, S, m);
        set_last_error(msg); return false;
    }
    return rows_ok("kid_sums", (long)S * m, (long)S * m, D);
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

size_t selftok_manifold_count_nn_f32_workspace_bytes(int M, int N, int D)
{
    if (M < 0 || N < 1) { set_last_error("manifold_count_nn: need M >= 0 queries and N >= 1 set rows"); return 0; }
    if (!rows_ok("manifold_count_nn", M, N, D)) return 0;
    const int ntiles = (N + BT - 1) / BT;
    const size_t parts = 2 * (size_t)(ntiles < GM_MAX_SPLIT ? ntiles : GM_MAX_SPLIT), rows = (size_t)(M > 0 ? M : 1);
    return align256(rows * sizeof(float)) + align256((size_t)N * sizeof(float)) + parts * rows * (sizeof(u64) + sizeof(int));
}

int selftok_manifold_count_nn_f32(const float* x, const float* a, const float* r2, int* count, float* nn_d2, int* nn_idx, void* workspace, size_t workspace_bytes,
                                  int M, int N, int D, int split, hipStream_t stream)
{
    const size_t need = selftok_manifold_count_nn_f32_workspace_bytes(M, N, D);
    if (!need) return SELFTOK_EINVAL;
    if (split < 0) { set_last_error("manifold_count_nn: split < 0 (0 = automatic)"); return SELFTOK_EINVAL; }
    if ((r2 == nullptr) != (count == nullptr)) { set_last_error("manifold_count_nn: count must be null exactly when r2 is (no radii, no count)"); return SELFTOK_EINVAL; }
    if (M == 0) return SELFTOK_OK;                                // no query: nothing to do (pointers may be null)
    if (!x || !a || !nn_d2 || !nn_idx || !workspace) { set_last_error("manifold_count_nn: null pointer"); return SELFTOK_EINVAL; }
    if (workspace_bytes < need) { set_last_error("manifold_count_nn: workspace smaller than selftok_manifold_count_nn_f32_workspace_bytes"); return SELFTOK_EINVAL; }
    if (((uintptr_t)x & 15) != 0 || ((uintptr_t)a & 15) != 0 || ((uintptr_t)workspace & 15) != 0 || ((uintptr_t)r2 & 3) != 0 || ((uintptr_t)count & 3) != 0 ||
        ((uintptr_t)nn_d2 & 3) != 0 || ((uintptr_t)nn_idx & 3) != 0) {
        set_last_error("manifold_count_nn: x, a and workspace must be 16-byte aligned, r2, count, nn_d2 and nn_idx 4-byte aligned"); return SELFTOK_EINVAL;
    }
    const int ntiles = (N + BT - 1) / BT, strips = (M + BT - 1) / BT;
    int s = pick_split(strips, ntiles, split);
    const int tps = (ntiles + s - 1) / s;
    s = (ntiles + tps - 1) / tps;                                 // every split holds at least one tile
    const size_t max_parts = 2 * (size_t)(ntiles < GM_MAX_SPLIT ? ntiles : GM_MAX_SPLIT);
    float* xnorm = (float*)workspace;
    float* anorm = (float*)((char*)workspace + align256((size_t)M * sizeof(float)));
    u64* keys = (u64*)((char*)anorm + align256((size_t)N * sizeof(float)));
    int* counts = (int*)(keys + max_parts * (size_t)M);
    hipLaunchKernelGGL(kdc_norm_kernel, dim3((unsigned)((M + NT - 1) / NT)), dim3(NT), 0, stream, x, xnorm, M, D);
    hipLaunchKernelGGL(kdc_norm_kernel, dim3((unsigned)((N + NT - 1) / NT)), dim3(NT), 0, stream, a, anorm, N, D);
    CountArgs p{x, xnorm, M, a, anorm, r2, N, D, tps, keys, counts};
    const dim3 grid((unsigned)strips, (unsigned)s);
    if (r2) hipLaunchKernelGGL(gm_count_nn_kernel<true>, grid, dim3(NT), 0, stream, p);
    else hipLaunchKernelGGL(gm_count_nn_kernel<false>, grid, dim3(NT), 0, stream, p);
    hipLaunchKernelGGL(gm_count_nn_finalize_kernel, dim3((unsigned)((M + NT - 1) / NT)), dim3(NT), 0, stream, (const u64*)keys, (const int*)counts, count, nn_d2, nn_idx,
                       M, 2 * s);
    return check_launch("manifold_count_nn kernels");
}

size_t selftok_kid_sums_f32_workspace_bytes(int S, int m, int D)
{
    if (!kid_ok(S, m, D)) return 0;
    const size_t T = (size_t)((m + BT - 1) / BT);
    return (size_t)S * 3 * T * T * sizeof(double);
}

int selftok_kid_sums_f32(const float* xs, const float* ys, double* sums, void* workspace, size_t workspace_bytes, int S, int m, int D, hipStream_t stream)
{
    const size_t need = selftok_kid_sums_f32_workspace_bytes(S, m, D);
    if (!need) return SELFTOK_EINVAL;
    if (!xs || !ys || !sums || !workspace) { set_last_error("kid_sums: null pointer"); return SELFTOK_EINVAL; }
    if (workspace_bytes < need) { set_last_error("kid_sums: workspace smaller than selftok_kid_sums_f32_workspace_bytes"); return SELFTOK_EINVAL; }
    if (((uintptr_t)xs & 15) != 0 || ((uintptr_t)ys & 15) != 0 || ((uintptr_t)workspace & 7) != 0 || ((uintptr_t)sums & 7) != 0) {
        set_last_error("kid_sums: xs and ys must be 16-byte aligned, sums and workspace 8-byte aligned"); return SELFTOK_EINVAL;
    }
    const int T = (m + BT - 1) / BT;
    hipLaunchKernelGGL(kid_tile_kernel, dim3((unsigned)(T * T), 3u, (unsigned)S), dim3(NT), 0, stream, xs, ys, (double*)workspace, m, D, T);
    hipLaunchKernelGGL(kid_finalize_kernel, dim3((unsigned)((3 * S + NT - 1) / NT)), dim3(NT), 0, stream, (const double*)workspace, sums, 3 * S, (long)T * T);
    return check_launch("kid_sums kernels");
}

}  // extern "C"
