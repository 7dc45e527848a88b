// Generative-model metrics on pool3 features and fc logits (include/selftok_hip_ext.h; selftoktokenizer_amd/genmetrics.py states the
// definitions, GEN_METRICS_DEFINITION; tests/gen_metrics_cases.py restates them in numpy fp64).
//
// Improved precision / recall (Kynkaanniemi et al. 2019): all pairwise SQUARED distances between two sets of fp32 rows, never stored.
//   csrc/gen_metrics_shared.h is the arithmetic of record of d2(u, v): one fp64 chain per norm rounded once, one k-ascending fmaf chain per dot product on
//   v_mfma_f32_32x32x2_f32, s = |u|^2 + |v|^2, d2 = s - 2 dot, clamped at +0.  Both entries below run that one body.
//   gm_pairs_kernel: one workgroup = one 128-row strip of the lane-side set against a contiguous run of 128-candidate tiles of the
//     register-side set (grid: row strips x column splits).  Per tile the K-loop over D stages both sides through LDS; the epilogue SELECTS:
//     RADIUS  every lane keeps the K smallest d2 of its row as a sorted list of fp32 bit patterns (non-negative floats order as unsigned
//             integers; 0xFFFFFFFF = empty), the candidate with the row's own index is skipped BY INDEX, a NaN distance is never inserted;
//             the two lane halves merge through the cross-lane network and the list goes to workspace[part][row][K], part = 2 * split + the
//             wave's candidate half.  gm_radius_finalize_kernel merges the parts: a merge of k-smallest lists is exact, any split gives
//             the same bits.  An entry k - 1 that is still empty (fewer than k non-NaN neighbours: a row holding a NaN) is written as NaN.
//     MEMBER  every lane ORs (d2 <= r2[candidate]) -- false against NaN -- into a flag; flags go to workspace[part][row] and
//             gm_member_finalize_kernel ORs the parts.  Order-independent.
//     Candidates past the end of the set are staged as zeros and masked by index: they never win a selection and never set a flag.
//   No atomics, no state: the outputs are functions of the inputs alone, whatever the split.
//
// Inception Score (fp64 from the fp32 logits on; every operation rounded on its own):
//   row n: m = max_y x_ny (fp32 compare), Z = sum_y exp((double)x_ny - m): lane l of one wave adds y = l, l + 64, ... ascending from +0.0,
//   the 64 lane sums are combined by the butterfly v = v + shfl_xor(v, o), o = 32, 16, .., 1 (commutative: every lane holds the same bits);
//   p_ny = exp((double)x_ny - m) / Z -- the SAME expression in the column sums and in the KL rows.
//   column means of split s (rows s * split_size .. ): chunks of 256 rows of the split, ascending rows from +0.0 inside a chunk, the chunk
//   sums combined by csrc/chunk_tree.h's binary-counter tree (the order of selftok_fid_stats), then / rows of the split.
//   kl[n] = sum_y p_ny * (log(p_ny) - log(q_sy)), q the column means of n's split; a term with p_ny == 0 is +0.0; lanes and butterfly as above.
#include "common.h"

#pragma clang fp contract(off)

#include "chunk_tree.h"
#include "gen_metrics_shared.h"
#include "selftok_hip_ext.h"
#include <stdio.h>

namespace selftok {
namespace {

using gm::BT; using gm::KT; using gm::LDS_STRIDE; using gm::NT; using gm::f32x16;

constexpr unsigned GM_EMPTY = 0xFFFFFFFFu;
constexpr int GM_MAX_SPLIT = 64;
constexpr long LIM = 1l << 31;

// one row per thread
__global__ void __launch_bounds__(NT) gm_norm_kernel(const float* __restrict__ x, float* __restrict__ norm, int N, int D)
{
    const int r = blockIdx.x * NT + threadIdx.x;
    if (r < N) norm[r] = gm::row_norm(x + (size_t)r * D, D);
}

// l[] ascending; after the call it holds the K smallest of (l[], key)
template <int K>
__device__ __forceinline__ void gm_insert(unsigned (&l)[K], unsigned key)
{
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const bool g = key < l[i];
        const unsigned keep = g ? key : l[i];
        key = g ? l[i] : key;
        l[i] = keep;
    }
}

struct PairArgs {
    const float* rows; const float* rnorm; int NR;                // lane side
    const float* cands; const float* cnorm; const float* cr2; int NC;      // register side; cr2: the candidates' radii (MEMBER)
    int D, tiles_per_split;
    void* ws;                                                     // RADIUS: unsigned [parts][NR][K]; MEMBER: int [parts][NR]
};

template <bool RADIUS, int K>
__global__ void __launch_bounds__(NT) gm_pairs_kernel(PairArgs a)
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
    unsigned best[2][K];
    bool hit[2] = {false, false};
#pragma unroll
    for (int ri = 0; ri < 2; ++ri)
#pragma unroll
        for (int i = 0; i < K; ++i) best[ri][i] = GM_EMPTY;

    for (int t = t_first; t < t_last; ++t) {
        const long c0 = (long)t * BT;
        __syncthreads();                                          // the previous tile's epilogue has read cn / cr
        if (tid < BT) {
            const long c = c0 + tid;
            cn[tid] = c < a.NC ? a.cnorm[c] : 0.0f;
            if (!RADIUS) cr[tid] = c < a.NC ? a.cr2[c] : 0.0f;
        }
        f32x16 acc[2][2];
        gm::tile_dots(a.rows, r0, a.NR, a.cands, c0, a.NC, a.D, Rs, Cs, acc);      // its barriers publish cn / cr
        const bool masked = c0 + BT > a.NC || (RADIUS && c0 == r0);               // a ragged last tile, or the tile that holds the rows themselves
#pragma unroll
        for (int ci = 0; ci < 2; ++ci) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int cl = cm + 32 * ci + 8 * q + 4 * fk;                       // candidates cl .. cl + 3 = accumulator registers 4 q .. 4 q + 3
                const float4 n4 = *(const float4*)(cn + cl);
                const float nn[4] = {n4.x, n4.y, n4.z, n4.w};
                float rr[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (!RADIUS) { const float4 r4 = *(const float4*)(cr + cl); rr[0] = r4.x; rr[1] = r4.y; rr[2] = r4.z; rr[3] = r4.w; }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const long cand = c0 + cl + j;
#pragma unroll
                    for (int ri = 0; ri < 2; ++ri) {
                        const float d = gm::pair_d2(rn[ri], nn[j], acc[ci][ri][4 * q + j]);
                        bool ok = true;
                        if (masked) ok = cand < a.NC && !(RADIUS && cand == r0 + rm + 32 * ri + fr);
                        if (RADIUS) {
                            const unsigned key = (ok && d == d) ? __float_as_uint(d) : GM_EMPTY;
                            if (key < best[ri][K - 1]) gm_insert<K>(best[ri], key);
                        } else {
                            hit[ri] = hit[ri] || (ok && d <= rr[j]);
                        }
                    }
                }
            }
        }
    }

    const int part = blockIdx.y * 2 + (wave >> 1);
#pragma unroll
    for (int ri = 0; ri < 2; ++ri) {
        const long r = r0 + rm + 32 * ri + fr;
        if (RADIUS) {
            unsigned other[K];
#pragma unroll
            for (int i = 0; i < K; ++i) other[i] = __shfl_xor(best[ri][i], 32, WAVE);
#pragma unroll
            for (int i = 0; i < K; ++i) gm_insert<K>(best[ri], other[i]);
            if (fk == 0 && r < a.NR) {
                unsigned* dst = (unsigned*)a.ws + ((size_t)part * a.NR + r) * K;
#pragma unroll
                for (int i = 0; i < K; ++i) dst[i] = best[ri][i];
            }
        } else {
            const int h = (int)hit[ri] | __shfl_xor((int)hit[ri], 32, WAVE);
            if (fk == 0 && r < a.NR) ((int*)a.ws)[(size_t)part * a.NR + r] = h;
        }
    }
}

template <int K>
__global__ void __launch_bounds__(NT) gm_radius_finalize_kernel(const unsigned* __restrict__ ws, float* __restrict__ r2, int N, int parts, int k)
{
    const int r = blockIdx.x * NT + threadIdx.x;
    if (r >= N) return;
    unsigned l[K];
#pragma unroll
    for (int i = 0; i < K; ++i) l[i] = ws[(size_t)r * K + i];
    for (int p = 1; p < parts; ++p) {
        const unsigned* src = ws + ((size_t)p * N + r) * K;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const unsigned key = src[i];
            if (key < l[K - 1]) gm_insert<K>(l, key);
        }
    }
    unsigned v = l[0];
#pragma unroll
    for (int i = 1; i < K; ++i) v = (i == k - 1) ? l[i] : v;
    r2[r] = v == GM_EMPTY ? __uint_as_float(0x7FC00000u) : __uint_as_float(v);
}

__global__ void __launch_bounds__(NT) gm_member_finalize_kernel(const int* __restrict__ ws, int* __restrict__ member, int M, int parts)
{
    const int r = blockIdx.x * NT + threadIdx.x;
    if (r >= M) return;
    int h = 0;
    for (int p = 0; p < parts; ++p) h |= ws[(size_t)p * M + r];
    member[r] = h;
}

int round_k(int k) { return k <= 1 ? 1 : (k <= 2 ? 2 : (k <= 4 ? 4 : 8)); }
size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// column splits: until the grid holds about four workgroups per compute unit, every split at least four tiles deep
int pick_split(int row_strips, int ntiles, int override_split)
{
    const int max_split = ntiles < GM_MAX_SPLIT ? ntiles : GM_MAX_SPLIT;
    int split = 1;
    while ((long)row_strips * split < 1024 && split * 2 <= max_split && ntiles / (split * 2) >= 4) split *= 2;
    if (override_split > 0) split = override_split < max_split ? override_split : max_split;
    return split;
}

bool pairs_shape_ok(const char* who, long n_rows, long n_cands, int D)
{
    char msg[256];
    if (D < 16 || D > 2048 || D % 16 != 0 || n_rows >= LIM / D || n_cands >= LIM / D) {
        snprintf(msg, sizeof msg, "%s: need D a multiple of 16 in 16 .. 2048 and rows * D below 2^31, got %ld and %ld rows, D %d", who, n_rows, n_cands, D);
        set_last_error(msg); return false;
    }
    return true;
}

// ---- Inception Score ----
constexpr int SCH = 256;                                          // rows per chunk of a split

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, WAVE);
    return v;
}

// one wave per row: stat[n] = {m, Z}
__global__ void __launch_bounds__(NT) is_rowstat_kernel(const float* __restrict__ x, double* __restrict__ stat, int N, int C)
{
    const int n = blockIdx.x * (NT / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    const float* row = x + (size_t)n * C;
    float m = -__builtin_inff();
    for (int y = lane; y < C; y += WAVE) { const float v = row[y]; m = v > m ? v : m; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float v = __shfl_xor(m, o, WAVE); m = v > m ? v : m; }
    double z = 0.0;
    for (int y = lane; y < C; y += WAVE) z = z + exp((double)row[y] - (double)m);
    z = wave_sum_f64(z);
    if (lane == 0) { stat[2 * (size_t)n] = (double)m; stat[2 * (size_t)n + 1] = z; }
}

__device__ __forceinline__ double is_p(float x, double m, double z) { return exp((double)x - m) / z; }

// grid (ceil(C / 64), splits * chunks_per_split): ws[g * C + y] = the chunk's sum of p[., y]
__global__ void __launch_bounds__(64) is_colsum_kernel(const float* __restrict__ x, const double* __restrict__ stat, double* __restrict__ ws, int N, int C,
                                                       int split_size, int cps)
{
    const int y = blockIdx.x * 64 + threadIdx.x;
    if (y >= C) return;
    const int s = blockIdx.y / cps, c = blockIdx.y - s * cps;
    const long lo = (long)s * split_size;
    const long hi = min(lo + split_size, (long)N);
    const long n0 = lo + (long)c * SCH, n1 = min(n0 + SCH, hi);
    double sum = 0.0;
    for (long n = n0; n < n1; ++n) sum = sum + is_p(x[(size_t)n * C + y], stat[2 * n], stat[2 * n + 1]);
    ws[(size_t)blockIdx.y * C + y] = sum;
}

// grid (ceil(C / 64), splits)
__global__ void __launch_bounds__(64) is_colmean_kernel(const double* __restrict__ ws, double* __restrict__ q, int N, int C, int split_size, int cps)
{
    const int y = blockIdx.x * 64 + threadIdx.x;
    if (y >= C) return;
    const int s = blockIdx.y;
    const long lo = (long)s * split_size;
    const long rows = min(lo + split_size, (long)N) - lo;
    const int chunks = (int)((rows + SCH - 1) / SCH);
    chunk_tree t; t.init();
    for (int c = 0; c < chunks; ++c) t.push(ws[((size_t)s * cps + c) * C + y]);
    q[(size_t)s * C + y] = t.total() / (double)rows;
}

// one wave per row
__global__ void __launch_bounds__(NT) is_kl_kernel(const float* __restrict__ x, const double* __restrict__ stat, const double* __restrict__ q, double* __restrict__ kl,
                                                   int N, int C, int split_size)
{
    const int n = blockIdx.x * (NT / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    const float* row = x + (size_t)n * C;
    const double* qs = q + (size_t)(n / split_size) * C;
    const double m = stat[2 * (size_t)n], z = stat[2 * (size_t)n + 1];
    double s = 0.0;
    for (int y = lane; y < C; y += WAVE) {
        const double p = is_p(row[y], m, z);
        const double term = p * (log(p) - log(qs[y]));
        s = s + (p == 0.0 ? 0.0 : term);
    }
    s = wave_sum_f64(s);
    if (lane == 0) kl[n] = s;
}

bool is_shape_ok(const char* who, int N, int C, int split_size)
{
    char msg[256];
    bool ok = N >= 1 && C >= 1 && split_size >= 1 && (long)N < LIM / C;
    if (ok) {
        const long S = ((long)N + split_size - 1) / split_size, cps = ((long)(split_size < N ? split_size : N) + SCH - 1) / SCH;
        ok = S * cps <= 65535 && S <= 65535;
    }
    if (!ok) {
        snprintf(msg, sizeof msg, "%s: need N, C, split_size >= 1, N * C below 2^31 and at most 65535 chunks of 256 rows over all splits, got N %d, C %d, split_size %d",
                 who, N, C, split_size);
        set_last_error(msg);
    }
    return ok;
}

int is_cps(int N, int split_size) { return ((split_size < N ? split_size : N) + SCH - 1) / SCH; }
int is_splits(int N, int split_size) { return (int)(((long)N + split_size - 1) / split_size); }

void launch_rowstat(const float* logits, double* stat, int N, int C, hipStream_t stream)
{
    hipLaunchKernelGGL(is_rowstat_kernel, dim3((unsigned)((N + NT / WAVE - 1) / (NT / WAVE))), dim3(NT), 0, stream, logits, stat, N, C);
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

size_t selftok_knn_radius_f32_workspace_bytes(int N, int D, int k)
{
    if (k < 1 || k > 8 || N <= k) { set_last_error("knn_radius: need 1 <= k <= 8 and N > k (a row has N - 1 neighbours)"); return 0; }
    if (!pairs_shape_ok("knn_radius", N, N, D)) return 0;
    const int ntiles = (N + BT - 1) / BT;
    const size_t parts = 2 * (size_t)(ntiles < GM_MAX_SPLIT ? ntiles : GM_MAX_SPLIT);
    return align256((size_t)N * sizeof(float)) + parts * (size_t)N * round_k(k) * sizeof(unsigned);
}

int selftok_knn_radius_f32(const float* a, float* r2, void* workspace, size_t workspace_bytes, int N, int D, int k, int split, hipStream_t stream)
{
    const size_t need = selftok_knn_radius_f32_workspace_bytes(N, D, k);
    if (!need) return SELFTOK_EINVAL;
    if (!a || !r2 || !workspace) { set_last_error("knn_radius: null pointer"); return SELFTOK_EINVAL; }
    if (split < 0) { set_last_error("knn_radius: split < 0 (0 = automatic)"); return SELFTOK_EINVAL; }
    if (workspace_bytes < need) { set_last_error("knn_radius: workspace smaller than selftok_knn_radius_f32_workspace_bytes"); return SELFTOK_EINVAL; }
    if (((uintptr_t)a & 15) != 0 || ((uintptr_t)workspace & 15) != 0 || ((uintptr_t)r2 & 3) != 0) {
        set_last_error("knn_radius: a and workspace must be 16-byte aligned, r2 4-byte aligned"); return SELFTOK_EINVAL;
    }
    float* norm = (float*)workspace;
    unsigned* lists = (unsigned*)((char*)workspace + align256((size_t)N * sizeof(float)));
    const int ntiles = (N + BT - 1) / BT;
    int s = pick_split(ntiles, ntiles, split);
    const int tps = (ntiles + s - 1) / s;
    s = (ntiles + tps - 1) / tps;                                 // every split holds at least one tile
    hipLaunchKernelGGL(gm_norm_kernel, dim3((unsigned)((N + NT - 1) / NT)), dim3(NT), 0, stream, a, norm, N, D);
    PairArgs p{a, norm, N, a, norm, nullptr, N, D, tps, lists};
    const dim3 grid((unsigned)ntiles, (unsigned)s), fin((unsigned)((N + NT - 1) / NT));
    const int kp = round_k(k);
    if (kp == 8) { hipLaunchKernelGGL((gm_pairs_kernel<true, 8>), grid, dim3(NT), 0, stream, p); hipLaunchKernelGGL(gm_radius_finalize_kernel<8>, fin, dim3(NT), 0, stream, lists, r2, N, 2 * s, k); }
    else if (kp == 4) { hipLaunchKernelGGL((gm_pairs_kernel<true, 4>), grid, dim3(NT), 0, stream, p); hipLaunchKernelGGL(gm_radius_finalize_kernel<4>, fin, dim3(NT), 0, stream, lists, r2, N, 2 * s, k); }
    else if (kp == 2) { hipLaunchKernelGGL((gm_pairs_kernel<true, 2>), grid, dim3(NT), 0, stream, p); hipLaunchKernelGGL(gm_radius_finalize_kernel<2>, fin, dim3(NT), 0, stream, lists, r2, N, 2 * s, k); }
    else { hipLaunchKernelGGL((gm_pairs_kernel<true, 1>), grid, dim3(NT), 0, stream, p); hipLaunchKernelGGL(gm_radius_finalize_kernel<1>, fin, dim3(NT), 0, stream, lists, r2, N, 2 * s, k); }
    return check_launch("knn_radius kernels");
}

size_t selftok_manifold_member_f32_workspace_bytes(int M, int N, int D)
{
    if (M < 0 || N < 1) { set_last_error("manifold_member: need M >= 0 queries and N >= 1 set rows"); return 0; }
    if (!pairs_shape_ok("manifold_member", M, N, D)) return 0;
    const int ntiles = (N + BT - 1) / BT;
    const size_t parts = 2 * (size_t)(ntiles < GM_MAX_SPLIT ? ntiles : GM_MAX_SPLIT);
    return align256((size_t)(M > 0 ? M : 1) * sizeof(float)) + align256((size_t)N * sizeof(float)) + parts * (size_t)(M > 0 ? M : 1) * sizeof(int);
}

int selftok_manifold_member_f32(const float* x, const float* a, const float* r2, int* member, void* workspace, size_t workspace_bytes, int M, int N, int D,
                                int split, hipStream_t stream)
{
    const size_t need = selftok_manifold_member_f32_workspace_bytes(M, N, D);
    if (!need) return SELFTOK_EINVAL;
    if (split < 0) { set_last_error("manifold_member: split < 0 (0 = automatic)"); return SELFTOK_EINVAL; }
    if (M == 0) return SELFTOK_OK;                                // no query: nothing to do (pointers may be null)
    if (!x || !a || !r2 || !member || !workspace) { set_last_error("manifold_member: null pointer"); return SELFTOK_EINVAL; }
    if (workspace_bytes < need) { set_last_error("manifold_member: workspace smaller than selftok_manifold_member_f32_workspace_bytes"); return SELFTOK_EINVAL; }
    if (((uintptr_t)x & 15) != 0 || ((uintptr_t)a & 15) != 0 || ((uintptr_t)workspace & 15) != 0 || ((uintptr_t)r2 & 3) != 0 || ((uintptr_t)member & 3) != 0) {
        set_last_error("manifold_member: x, a and workspace must be 16-byte aligned, r2 and member 4-byte aligned"); return SELFTOK_EINVAL;
    }
    float* xnorm = (float*)workspace;
    float* anorm = (float*)((char*)workspace + align256((size_t)M * sizeof(float)));
    int* flags = (int*)((char*)anorm + align256((size_t)N * sizeof(float)));
    const int ntiles = (N + BT - 1) / BT, strips = (M + BT - 1) / BT;
    int s = pick_split(strips, ntiles, split);
    const int tps = (ntiles + s - 1) / s;
    s = (ntiles + tps - 1) / tps;
    hipLaunchKernelGGL(gm_norm_kernel, dim3((unsigned)((M + NT - 1) / NT)), dim3(NT), 0, stream, x, xnorm, M, D);
    hipLaunchKernelGGL(gm_norm_kernel, dim3((unsigned)((N + NT - 1) / NT)), dim3(NT), 0, stream, a, anorm, N, D);
    PairArgs p{x, xnorm, M, a, anorm, r2, N, D, tps, flags};
    hipLaunchKernelGGL((gm_pairs_kernel<false, 1>), dim3((unsigned)strips, (unsigned)s), dim3(NT), 0, stream, p);
    hipLaunchKernelGGL(gm_member_finalize_kernel, dim3((unsigned)((M + NT - 1) / NT)), dim3(NT), 0, stream, (const int*)flags, member, M, 2 * s);
    return check_launch("manifold_member kernels");
}

size_t selftok_is_colmean_workspace_bytes(int N, int C, int split_size)
{
    if (!is_shape_ok("is_colmean", N, C, split_size)) return 0;
    return (size_t)N * 2 * sizeof(double) + (size_t)is_splits(N, split_size) * is_cps(N, split_size) * (size_t)C * sizeof(double);
}

int selftok_is_colmean(const float* logits, double* colmean, void* workspace, size_t workspace_bytes, int N, int C, int split_size, hipStream_t stream)
{
    const size_t need = selftok_is_colmean_workspace_bytes(N, C, split_size);
    if (!need) return SELFTOK_EINVAL;
    if (!logits || !colmean || !workspace) { set_last_error("is_colmean: null pointer"); return SELFTOK_EINVAL; }
    if (workspace_bytes < need) { set_last_error("is_colmean: workspace smaller than selftok_is_colmean_workspace_bytes"); return SELFTOK_EINVAL; }
    if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)colmean & 7) != 0 || ((uintptr_t)logits & 3) != 0) {
        set_last_error("is_colmean: workspace and colmean must be 8-byte aligned, logits 4-byte aligned"); return SELFTOK_EINVAL;
    }
    double* stat = (double*)workspace;
    double* sums = stat + 2 * (size_t)N;
    const int S = is_splits(N, split_size), cps = is_cps(N, split_size);
    launch_rowstat(logits, stat, N, C, stream);
    hipLaunchKernelGGL(is_colsum_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)(S * cps)), dim3(64), 0, stream, logits, (const double*)stat, sums, N, C, split_size, cps);
    hipLaunchKernelGGL(is_colmean_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)S), dim3(64), 0, stream, (const double*)sums, colmean, N, C, split_size, cps);
    return check_launch("is_colmean kernels");
}

size_t selftok_is_kl_rows_workspace_bytes(int N, int C, int split_size)
{
    if (!is_shape_ok("is_kl_rows", N, C, split_size)) return 0;
    return (size_t)N * 2 * sizeof(double);
}

int selftok_is_kl_rows(const float* logits, const double* colmean, double* kl, void* workspace, size_t workspace_bytes, int N, int C, int split_size, hipStream_t stream)
{
    const size_t need = selftok_is_kl_rows_workspace_bytes(N, C, split_size);
    if (!need) return SELFTOK_EINVAL;
    if (!logits || !colmean || !kl || !workspace) { set_last_error("is_kl_rows: null pointer"); return SELFTOK_EINVAL; }
    if (workspace_bytes < need) { set_last_error("is_kl_rows: workspace smaller than selftok_is_kl_rows_workspace_bytes"); return SELFTOK_EINVAL; }
    if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)colmean & 7) != 0 || ((uintptr_t)kl & 7) != 0 || ((uintptr_t)logits & 3) != 0) {
        set_last_error("is_kl_rows: workspace, colmean and kl must be 8-byte aligned, logits 4-byte aligned"); return SELFTOK_EINVAL;
    }
    double* stat = (double*)workspace;
    launch_rowstat(logits, stat, N, C, stream);
    hipLaunchKernelGGL(is_kl_kernel, dim3((unsigned)((N + NT / WAVE - 1) / (NT / WAVE))), dim3(NT), 0, stream, logits, (const double*)stat, colmean, kl, N, C, split_size);
    return check_launch("is_kl_rows kernels");
}

}  // extern "C"
