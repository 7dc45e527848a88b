// Selftok VQ lookup, the k best codes of every row with their exact scores (k <= 8) for gfx950 (MI355X).
//
// For row n: x = l2norm16(z[n]) (unless SELFTOK_PRENORMED), s[c] = the canonical k-ordered fp32 FMA chain of vq.hip's header
// (oracle/selftok_oracle.c: score16).  The result is the first k entries of all codes ordered by
//   * score descending;
//   * equal scores by ascending code index, -0.0 == +0.0 (a zero score is written as +0.0);
//   * NaN scores before every number, among themselves by ascending index (written as the quiet NaN 0x7FC00000).
// Column 0 is therefore, bit for bit, the (ids, best) of selftok_vq_encode_packed_f32.
//
// One 64-bit key per (row, code) carries the whole order:  key = orderable(score) << 32 | (0xFFFFFFFF - code), NaN scores
// with the high word 0xFFFFFFFF: a larger unsigned key is an earlier entry, and keys of different codes are never equal.
//
// vq_topk_kernel<RT, K>: the scores come from v_mfma_f32_32x32x2_f32 on the packed code book -- operand layout, LDS staging and
//   row blocking are vq_mfma_kernel's, so the scores are the canonical ones and no error window is needed.  Every lane stream
//   (one wave half of one code split: 16 codes of each of its tiles) keeps its K best keys sorted in registers.  A stream meets
//   its codes in ascending index order, so on the fast path a score enters the list only if it is STRICTLY greater than the
//   stream's current K-th score: one float compare per score (after one compare per tile against the tile maximum), and the
//   rare pass is a register insertion of K compare-exchanges.  Waves that hold a non-finite row, or any wave when the pack step
//   flagged the code book, build the key of every score and compare keys instead (NaN-aware, exact).  At the end the two wave
//   halves of a row exchange their lists through the cross-lane network and merge them: the workspace receives K keys per
//   (code split, row).
// vq_topk_finalize_kernel<IdT, K>: one thread per row merges the splits' sorted lists and writes ids[N, k], scores[N, k].
//
// This file is compiled with -ffp-contract=off.
#include "common.h"
#include "selftok_hip_ext.h"   // the C ABI declared there must match the definitions below
#include "vq_shared.h"

namespace selftok {

// below the key of every real code: orderable(-inf) in the high word, and a low word no code has (code 0xFFFFFFFF does not exist)
constexpr unsigned long long TOPK_EMPTY = 0x007FFFFF00000000ull;
constexpr int TOPK_MAX_SPLIT = 64;

__device__ __forceinline__ unsigned long long topk_key(float s, uint32_t code)
{
    float v = s;
    if (v == 0.0f) v = 0.0f;                                    // -0 -> +0: equal scores, the lower index is first
    const uint32_t hi = (s != s) ? KEY_NAN : f32_orderable(v);
    return ((unsigned long long)hi << 32) | (uint32_t)(~code);
}

// l[] is sorted descending; after the call it holds the K largest of (l[], key), sorted.  Straight-line: the list stays in registers.
template <int K>
__device__ __forceinline__ void topk_insert(unsigned long long (&l)[K], unsigned long long key)
{
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const bool g = key > l[i];
        const unsigned long long up = g ? key : l[i];
        key = g ? l[i] : key;
        l[i] = up;
    }
}

// score of the list's last entry as a float (TOPK_EMPTY -> -inf).  Fast path only: no NaN key is ever in the list there.
template <int K>
__device__ __forceinline__ float topk_threshold(const unsigned long long (&l)[K]) { return f32_from_orderable((uint32_t)(l[K - 1] >> 32)); }

// code index of accumulator register r of lane half `half` in tile `tile` (32x32 MFMA C layout: 4 rows every 8, halves 4 apart)
__device__ __forceinline__ uint32_t topk_code(int tile, int half, int r) { return (uint32_t)(tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * half); }

template <int K, bool EXACT>
__device__ __forceinline__ void topk_scan(unsigned long long (&l)[K], float& thr, const f32x16& acc, int tile, int half)
{
    if (EXACT) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned long long key = topk_key(acc[r], topk_code(tile, half, r));
            if (key > l[K - 1]) topk_insert<K>(l, key);
        }
        return;
    }
    float m = acc[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) m = __builtin_fmaxf(m, acc[r]);
    if (m > thr) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float s = acc[r];
            if (s > thr) {            // strict: this stream's earlier codes have lower indices and stay ahead on equal scores
                topk_insert<K>(l, topk_key(s, topk_code(tile, half, r)));
                thr = topk_threshold<K>(l);
            }
        }
    }
}

__device__ __forceinline__ unsigned long long topk_shfl_xor32(unsigned long long k)
{
    uint32_t lo = (uint32_t)k, hi = (uint32_t)(k >> 32);
    lo = __shfl_xor(lo, 32, WAVE);
    hi = __shfl_xor(hi, 32, WAVE);
    return ((unsigned long long)hi << 32) | lo;
}

template <int RT, int K>
__global__ __launch_bounds__(256) void vq_topk_kernel(const float* __restrict__ z, const float* __restrict__ packed,
                                                      unsigned long long* __restrict__ partial, int N, int C,
                                                      int tiles_per_split, int normalize)
{
    __shared__ __attribute__((aligned(16))) float s_frag[2][M_CH * 512];     // staged as in vq_mfma_kernel: LDS-DMA, double buffered

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int row0 = (blockIdx.x * 4 + wave) * 32 * RT;

    // B operands: B[k][j] = x[row j][k]; lane (half, col) holds k = 2m + half of row col
    float b[RT][8];
    bool xbad = false;
    const uint32_t hmask = half ? 0xFFFFFFFFu : 0u;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        float zz[D], xx[D];
        int r = row0 + t * 32 + col;
        r = r < N ? r : N - 1;                       // clamp: out-of-range lanes redo the last row, never stored
        load_row16(z + (size_t)r * D, zz);
        if (normalize) l2norm16(zz, xx);
        else {
#pragma unroll
            for (int k = 0; k < D; ++k) xx[k] = zz[k];
        }
#pragma unroll
        for (int k = 0; k < D; ++k) xbad |= suspicious(xx[k]);
#pragma unroll
        for (int m = 0; m < 8; ++m)   // bit-select (not an indexed load: that would push xx[] into scratch)
            b[t][m] = __uint_as_float((__float_as_uint(xx[2 * m + 1]) & hmask) | (__float_as_uint(xx[2 * m]) & ~hmask));
    }
    // metadata word of the packed image: bit 0 = a code element is non-finite / absurd
    const bool slow = __any(xbad) || ((reinterpret_cast<const uint32_t*>(packed)[(size_t)C * D] & 1u) != 0u);

    const int ntiles_total = C >> 5;
    const int tile_first = blockIdx.y * tiles_per_split;
    int tile_last = tile_first + tiles_per_split;
    if (tile_last > ntiles_total) tile_last = ntiles_total;
    const int nt = tile_last - tile_first;

    unsigned long long best[RT][K];
    float thr[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        thr[t] = -__builtin_inff();
#pragma unroll
        for (int i = 0; i < K; ++i) best[t][i] = TOPK_EMPTY;
    }

    // this wave's share of a chunk: pieces wave, wave+4, ... of the 2*M_CH (tile, part) pieces, 1 KiB each
    auto stage = [&](int chunk, int buf) {
#pragma unroll
        for (int pi = wave; pi < 2 * M_CH; pi += 4) {
            int tl = chunk * M_CH + (pi >> 1);
            tl = tl < nt ? tl : nt - 1;                                   // ragged last chunk: re-read the last tile
            const float* src = packed + (size_t)(tile_first + tl) * 512 + (pi & 1) * 256 + lane * 4;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(&s_frag[buf][pi * 256]), 16, 0, 0);
        }
    };

    if (nt > 0) {
        const int nchunks = (nt + M_CH - 1) / M_CH;
        stage(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int c = 0; c < nchunks; ++c) {
            const int buf = c & 1;
            if (c + 1 < nchunks) stage(c + 1, buf ^ 1);                   // DMA the next chunk behind this chunk's MFMAs
            const int base = c * M_CH;
            for (int j = 0; j < M_CH && base + j < nt; ++j) {
                const float4 lo = *reinterpret_cast<const float4*>(&s_frag[buf][j * 512 + lane * 4]);
                const float4 hi = *reinterpret_cast<const float4*>(&s_frag[buf][j * 512 + 256 + lane * 4]);
                const float a[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                f32x16 acc[RT];
#pragma unroll
                for (int t = 0; t < RT; ++t) acc[t] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int m = 0; m < 8; ++m)       // k = 2m (lanes 0-31), 2m+1 (lanes 32-63): k-ordered chain per accumulator
#pragma unroll
                    for (int t = 0; t < RT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], b[t][m], acc[t], 0, 0, 0);
                const int tile = tile_first + base + j;
                if (slow) {
#pragma unroll
                    for (int t = 0; t < RT; ++t) topk_scan<K, true>(best[t], thr[t], acc[t], tile, half);
                } else {
#pragma unroll
                    for (int t = 0; t < RT; ++t) topk_scan<K, false>(best[t], thr[t], acc[t], tile, half);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // my DMAs of chunk c+1 have landed
            __syncthreads();                                              // everyone's have, and chunk c's buffer is free
        }
    }

    // merge the two wave halves of every row (lanes col and col + 32), the lower half writes K keys per (split, row)
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        unsigned long long other[K];
#pragma unroll
        for (int i = 0; i < K; ++i) other[i] = topk_shfl_xor32(best[t][i]);
#pragma unroll
        for (int i = 0; i < K; ++i) topk_insert<K>(best[t], other[i]);
        const int r = row0 + t * 32 + col;
        if (half == 0 && r < N) {
            unsigned long long* dst = partial + ((size_t)blockIdx.y * N + r) * K;
#pragma unroll
            for (int i = 0; i < K; ++i) dst[i] = best[t][i];
        }
    }
}

template <typename IdT, int K>
__global__ __launch_bounds__(256) void vq_topk_finalize_kernel(const unsigned long long* __restrict__ partial, IdT* __restrict__ ids,
                                                               float* __restrict__ scores, int N, int nsplit, int k)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    unsigned long long l[K];
#pragma unroll
    for (int i = 0; i < K; ++i) l[i] = partial[(size_t)r * K + i];
    for (int s = 1; s < nsplit; ++s) {
        const unsigned long long* src = partial + ((size_t)s * N + r) * K;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const unsigned long long key = src[i];
            if (key > l[K - 1]) topk_insert<K>(l, key);
        }
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
        if (i < k) {
            const uint32_t hi = (uint32_t)(l[i] >> 32);
            ids[(size_t)r * k + i] = (IdT)(~(uint32_t)l[i]);
            scores[(size_t)r * k + i] = (hi == KEY_NAN) ? __uint_as_float(0x7FC00000u) : f32_from_orderable(hi);
        }
    }
}

static int topk_round_k(int k) { return k <= 1 ? 1 : (k <= 2 ? 2 : (k <= 4 ? 4 : 8)); }

template <int RT, int K>
static void topk_launch(dim3 grid, hipStream_t stream, const float* z, const float* packed, unsigned long long* partial, int N, int C, int tps, int norm)
{
    hipLaunchKernelGGL((vq_topk_kernel<RT, K>), grid, dim3(256), 0, stream, z, packed, partial, N, C, tps, norm);
}
template <int K>
static void topk_launch_rt(int rt, dim3 grid, hipStream_t stream, const float* z, const float* packed, unsigned long long* partial, int N, int C, int tps, int norm)
{
    if (rt == 4) topk_launch<4, K>(grid, stream, z, packed, partial, N, C, tps, norm);
    else if (rt == 2) topk_launch<2, K>(grid, stream, z, packed, partial, N, C, tps, norm);
    else topk_launch<1, K>(grid, stream, z, packed, partial, N, C, tps, norm);
}
template <int K>
static void topk_finalize(hipStream_t stream, const unsigned long long* partial, void* ids, float* scores, int N, int nsplit, int k, bool i32)
{
    const dim3 grid((N + 255) / 256), block(256);
    if (i32) hipLaunchKernelGGL((vq_topk_finalize_kernel<int32_t, K>), grid, block, 0, stream, partial, (int32_t*)ids, scores, N, nsplit, k);
    else hipLaunchKernelGGL((vq_topk_finalize_kernel<long long, K>), grid, block, 0, stream, partial, (long long*)ids, scores, N, nsplit, k);
}

}  // namespace selftok

using namespace selftok;

extern "C" {

// nsplit_max x N x kpad keys of 8 bytes: nsplit_max = min(64, C / 32) code splits, kpad = k rounded up to 1, 2, 4 or 8
size_t selftok_vq_topk_workspace_bytes(int N, int C, int k)
{
    if (k < 1 || k > 8 || C <= 0 || (C & 31) || N < 0) { set_last_error("vq_topk_workspace_bytes: need 1 <= k <= 8, C > 0, C % 32 == 0, N >= 0"); return 0; }
    const int ntiles = C >> 5;
    const size_t nsplit_max = ntiles < TOPK_MAX_SPLIT ? ntiles : TOPK_MAX_SPLIT;
    return nsplit_max * (size_t)(N > 0 ? N : 1) * (size_t)topk_round_k(k) * sizeof(unsigned long long);
}

int selftok_vq_topk_packed_f32(const float* z, const float* packed, void* ids, float* scores, void* workspace,
                               int N, int C, int Dm, int k, int flags, hipStream_t stream)
{
    if (k < 1 || k > 8) { set_last_error("vq_topk_packed: k must be in 1..8"); return SELFTOK_EINVAL; }
    if (Dm != D || C <= 0 || (C & 31)) { set_last_error("vq_topk_packed: need D == 16 and C % 32 == 0"); return SELFTOK_EINVAL; }
    if (N < 0) { set_last_error("vq_topk_packed: N < 0"); return SELFTOK_EINVAL; }
    if (N == 0) return SELFTOK_OK;                     // empty batch: nothing to do (pointers may be null)
    if (!z || !packed || !ids || !scores || !workspace) { set_last_error("vq_topk_packed: null pointer"); return SELFTOK_EINVAL; }
    unsigned long long* partial = (unsigned long long*)workspace;
    const int ntiles = C >> 5;
    const int kp = topk_round_k(k);
    // launch shape (results never depend on it): two row blocks per wave on large batches, code splits until ~4 workgroups per CU
    int rt = N >= 16384 ? 2 : 1;
    { const int f_rt = (flags >> 8) & 0xF; if (f_rt == 1 || f_rt == 2 || f_rt == 4) rt = f_rt; }     // SELFTOK_VQ_RT
    const int row_blocks = (N + 128 * rt - 1) / (128 * rt);
    const int max_split = ntiles < TOPK_MAX_SPLIT ? ntiles : TOPK_MAX_SPLIT;
    int split = 1;
    while (row_blocks * split < 1024 && split * 2 <= max_split && ntiles / (split * 2) >= 8) split *= 2;
    { const int f_split = (flags >> 16) & 0xFF; if (f_split > 0 && f_split <= max_split) split = f_split; }   // SELFTOK_VQ_SPLIT
    const int tps = (ntiles + split - 1) / split;
    split = (ntiles + tps - 1) / tps;                  // every split holds at least one tile: every lane stream sees >= 16 codes >= k
    const int norm = (flags & SELFTOK_PRENORMED) ? 0 : 1;
    const dim3 grid(row_blocks, split);
    if (kp == 8) topk_launch_rt<8>(rt, grid, stream, z, packed, partial, N, C, tps, norm);
    else if (kp == 4) topk_launch_rt<4>(rt, grid, stream, z, packed, partial, N, C, tps, norm);
    else if (kp == 2) topk_launch_rt<2>(rt, grid, stream, z, packed, partial, N, C, tps, norm);
    else topk_launch_rt<1>(rt, grid, stream, z, packed, partial, N, C, tps, norm);
    int rc = check_launch("vq_topk_kernel");
    if (rc) return rc;
    const bool i32 = (flags & SELFTOK_IDS_I32) != 0;
    if (kp == 8) topk_finalize<8>(stream, partial, ids, scores, N, split, k, i32);
    else if (kp == 4) topk_finalize<4>(stream, partial, ids, scores, N, split, k, i32);
    else if (kp == 2) topk_finalize<2>(stream, partial, ids, scores, N, split, k, i32);
    else topk_finalize<1>(stream, partial, ids, scores, N, split, k, i32);
    return check_launch("vq_topk_finalize_kernel");
}

}  // extern "C"
