// Token scorer: one row of AR logits over a window of C codes and ONE KNOWN target id -> the target's log-probability, its rank, the row's first code and
// its entropy (include/selftok_hip_ext.h states the arithmetic of record, steps 1 - 4 of the sampler's and the scorer's own block; selftoktokenizer_amd/
// sampling.py is the host side; tests/token_score_cases.py restates every step in numpy).
//
// A workgroup of 512 threads owns a row; the grid is one workgroup per row (x = min(R, 65536), y the rest), nothing persistent.  Thread t owns the 4-code
// chunks t, t + 512, t + 1024, ..: one 16-byte load per chunk for fp32 logits, one 8-byte load for bf16; the up to three codes of the partial chunk at the window's end are
// read code by code, by thread 0.  At C <= 32768 the row is read from memory ONCE and its keys stay in registers (tok_score_kernel<16, .>: 64 keys per thread; <2, .> for
// C <= 4096: 8 keys, so that a small vocabulary does not pay for fourteen empty chunks); above that the chunks are read a second time through the L2
// (tok_score_kernel<0, .>).  Two sweeps and two barriers per row: (1) keys, the maximum, NaN / +inf; (2) per code the integer mass q, the integer entropy
// term h, "is this code ahead of the target" and the lowest index at the maximum key.  Every reduction is a maximum, an integer sum or a minimum, over
// shuffles and LDS atomics: any order gives the same bits.  The floating-point operations are the guidance / temperature products, the mass polynomial, two
// fp64 products and a truncation per code for h, and thread 0's fp64 logarithm and quotient.  No inline assembly, no scratch, no state, no workspace.
#include "common.h"
#include "selftok_hip_ext.h"
#include <math.h>
#include <stdio.h>

namespace selftok {
namespace {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned short u16;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

constexpr int NT = 512;                                           // threads per row
constexpr int REG_CH = 16;                                        // chunks of 4 codes a thread keeps in registers: 16 * 4 * 512 = 32768
constexpr int SMALL_CH = 2;                                       // 2 * 4 * 512 = 4096
constexpr int MAX_C = 65536;
constexpr int GRID_X = 65536;                                     // rows per grid row
constexpr u32 KEY_NEG_INF = 0x007FFFFFu;                          // f32_orderable(-inf)
constexpr u32 KEY_NONE = 0xFFFFFFFFu;                             // above the key of every logit of a good row: nothing is ahead of it

struct ScoreArgs {
    const void* logits; const void* uncond; const void* ids;
    float* logprob; u64* mass; int* rank; int* top_id; float* entropy; u32* bad; u32* ignored;
    long row_stride, offset, id_seq_stride, id_step_stride;
    int R, C, id_bytes, S;
    float cfg_scale, inv_T;
};

struct Shared {
    u64 qtot, hsum;
    u32 maxkey, flags, ahead, first;
    u32 ktail[4];                                                 // the keys of the partial chunk's up to three codes (0: no such code)
};

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int o)
{
    const u32 lo = __shfl_xor((u32)v, o, WAVE), hi = __shfl_xor((u32)(v >> 32), o, WAVE);
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ float widen(u16 h) { return __uint_as_float((u32)h << 16); }

// guidance and temperature: difference, product, sum, product -- four roundings, none fused (the sampler's step 1)
__device__ __forceinline__ float scaled_logit(float lc, float lu, bool guided, float s, float inv_T)
{
    float l = lc;
    if (guided) {
        const float diff = lc - lu;
        const float prod = s * diff;
        l = lu + prod;
    }
    return l * inv_T;
}

// the monotone uint32 key of a logit (-0.0 as +0.0); a NaN or +inf sets badf (the sampler's step 3)
__device__ __forceinline__ u32 key_of(float l, u32& badf)
{
    u32 u = __float_as_uint(l);
    if ((u & 0x7FFFFFFFu) == 0u) u = 0u;
    badf |= ((u & 0x7FFFFFFFu) > 0x7F800000u || u == 0x7F800000u) ? 1u : 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the integer mass of a code d = l - m below the row maximum (the sampler's step 4, the same constants): exactly 2^32 at d = 0, 0 below -24, for -inf and
// for the NaN that a code past the window decodes to.  Branch-free -- the polynomial runs on dd = 0 where the mass is 0 -- so that a chunk of the sweep is ONE
// basic block and its scheduling barrier holds: with a branch per code the compiler computed all 64 masses of a thread first and kept them (1 KB of scratch).
// dd is handed back for the entropy term: q * (-dd) is 0 wherever q is.
__device__ __forceinline__ u64 mass_of(float d, float& dd)
{
    const bool ok = d >= -24.0f;
    dd = ok ? d : 0.0f;
    const float n = rintf(dd * 1.4426950408889634f);
    const float r = (dd - n * 0.693145751953125f) - n * 1.428606765330187045e-06f;
    float p = (float)(1.0 / 720.0) * r + (float)(1.0 / 120.0);
    p = p * r + (float)(1.0 / 24.0);
    p = p * r + (float)(1.0 / 6.0);
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    const float scale = __uint_as_float((u32)((int)n + 32 + 127) << 23);      // 2^(n + 32), n + 32 in [-3, 32]: the product is exact
    const u64 q = (u64)(p * scale);
    return ok ? q : 0ull;
}

template <bool BF16>
__device__ __forceinline__ float logit_at(const ScoreArgs& a, size_t row, u32 idx)
{
    const bool guided = a.uncond != nullptr;
    float lc, lu = 0.0f;
    if (BF16) {
        lc = widen(((const u16*)a.logits)[row + idx]);
        if (guided) lu = widen(((const u16*)a.uncond)[row + idx]);
    } else {
        lc = ((const float*)a.logits)[row + idx];
        if (guided) lu = ((const float*)a.uncond)[row + idx];
    }
    return scaled_logit(lc, lu, guided, a.cfg_scale, a.inv_T);
}

// the keys of the whole chunk j (codes 4 j .. 4 j + 3 < C): one vector load per input; a chunk at or past the window's last, partial chunk gets keys 0: below
// every real key, a key 0 decodes to a NaN whose mass is 0, it is ahead of no target and never the maximum.  Such a chunk reads chunk 0 instead of nothing
// (the caller has checked C >= 4): without a branch the sixteen chunks of a thread are one basic block, in which the scheduling barriers hold -- with one the
// compiler issued all sixteen loads (thirty-two with guidance) before the first key and spilled.  The up to three codes of the partial chunk are thread 0's,
// read code by code.
template <bool BF16, bool GUIDED>
__device__ __forceinline__ void load_chunk(const ScoreArgs& a, size_t row, int j, u32 k[4], u32& badf)
{
    const u32 i0 = 4u * (u32)j;
    const u32 in = (u32)((int)(i0 + 3u - (u32)a.C) >> 31);        // all ones inside the window; a vector mask, not sixteen scalar ones held across the loads
    const size_t at = row + (i0 & in);
    float lc[4], lu[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (BF16) {
        const u16x4 v = *(const u16x4*)((const u16*)a.logits + at);
#pragma unroll
        for (int e = 0; e < 4; ++e) lc[e] = widen(v[e]);
        if (GUIDED) {
            const u16x4 w = *(const u16x4*)((const u16*)a.uncond + at);
#pragma unroll
            for (int e = 0; e < 4; ++e) lu[e] = widen(w[e]);
        }
    } else {
        const f32x4 v = *(const f32x4*)((const float*)a.logits + at);
#pragma unroll
        for (int e = 0; e < 4; ++e) lc[e] = v[e];
        if (GUIDED) {
            const f32x4 w = *(const f32x4*)((const float*)a.uncond + at);
#pragma unroll
            for (int e = 0; e < 4; ++e) lu[e] = w[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        u32 f = 0u;
        const u32 key = key_of(scaled_logit(lc[e], lu[e], GUIDED, a.cfg_scale, a.inv_T), f);
        k[e] = key & in;
        badf |= f & in;
    }
}

template <int NCH, bool BF16, bool GUIDED>
__global__ void __launch_bounds__(NT, 4) tok_score_kernel(const ScoreArgs a)
{
    __shared__ Shared sh;
    const long r = (long)blockIdx.y * GRID_X + (long)blockIdx.x;
    if (r >= (long)a.R) return;                                   // the last grid row: block-uniform
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t row = (size_t)r * (size_t)a.row_stride + (size_t)a.offset;
    const int n_it = NCH ? NCH : (a.C + 4 * NT - 1) / (4 * NT);
    const u32 tail0 = (u32)a.C & ~3u;                             // the first code of the partial chunk

    if (tid == 0) { sh.qtot = 0ull; sh.hsum = 0ull; sh.maxkey = 0u; sh.flags = 0u; sh.ahead = 0u; sh.first = 0xFFFFFFFFu; sh.ktail[0] = 0u; sh.ktail[1] = 0u; sh.ktail[2] = 0u; }

    // the target: every thread reads the same element
    const long io = (r / a.S) * a.id_seq_stride + (r % a.S) * a.id_step_stride;
    const long long tv_v = a.id_bytes == 8 ? ((const long long*)a.ids)[io] : (long long)((const int*)a.ids)[io];
    const long long tv = (long long)(((u64)(u32)__builtin_amdgcn_readfirstlane((int)((u64)tv_v >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)tv_v));
    __syncthreads();

    // ---- the one read of the row: keys, maximum, NaN / +inf ----
    u32 kreg[NCH ? NCH : 1][4];
    u32 mx = 0u, badf = 0u;
    auto first_read = [&](int i) {
        u32 k[4];
        load_chunk<BF16, GUIDED>(a, row, tid + NT * i, k, badf);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (NCH) kreg[NCH ? i : 0][e] = k[e];
            mx = k[e] > mx ? k[e] : mx;
        }
        if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // four chunks' loads in flight per thread (eight with guidance), not all sixteen
    };
    if (a.C >= 4) {                                               // block-uniform: chunk 0 is whole
        if constexpr (NCH > 0) {
#pragma unroll
            for (int i = 0; i < NCH; ++i) first_read(i);
        } else {
            for (int i = 0; i < n_it; ++i) first_read(i);
        }
    } else if constexpr (NCH > 0) {
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) kreg[i][e] = 0u;
    }
    if (tid == 0) {
#pragma unroll
        for (int e = 0; e < 3; ++e)
            if (tail0 + e < (u32)a.C) {
                const u32 key = key_of(logit_at<BF16>(a, row, tail0 + e), badf);
                sh.ktail[e] = key;
                mx = key > mx ? key : mx;
            }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u32 v = __shfl_xor(mx, o, WAVE); mx = v > mx ? v : mx; }
    if (lane == 0) atomicMax(&sh.maxkey, mx);
    if (__ballot(badf != 0u) != 0ull && lane == 0) atomicOr(&sh.flags, 1u);
    __syncthreads();

    const u32 maxkey = (u32)__builtin_amdgcn_readfirstlane((int)sh.maxkey);               // block-uniform values belong in scalar registers
    if (sh.flags != 0u || maxkey <= KEY_NEG_INF || tv >= (long long)a.C) {             // a bad row: block-uniform
        if (tid == 0) {
            a.logprob[r] = __uint_as_float(0x7FC00000u);
            a.entropy[r] = __uint_as_float(0x7FC00000u);
            a.rank[r] = -1; a.top_id[r] = -1;
            a.mass[2 * (size_t)r] = 0ull; a.mass[2 * (size_t)r + 1] = 0ull;
            atomicAdd(a.bad, 1u);
        }
        return;
    }
    const float m = f32_from_orderable(maxkey);
    const bool scored = tv >= 0;
    const u32 tidx = scored ? (u32)tv : 0u;
    u32 tkey = KEY_NONE;
    if (scored) { u32 f = 0u; tkey = (u32)__builtin_amdgcn_readfirstlane((int)key_of(logit_at<BF16>(a, row, tidx), f)); }

    // ---- the sweep: mass, entropy term, codes ahead of the target, the first code of the order ----
    u64 q_sum = 0ull, h_sum = 0ull;
    u32 ahead = 0u, first = 0xFFFFFFFFu;
    auto code = [&](u32 key, u32 idx) {
        const float d = f32_from_orderable(key) - m;
        float dd;
        const u64 q = mass_of(d, dd);
        q_sum += q;
        h_sum += (u64)((double)q * (double)(-dd) * 65536.0);                 // 0 where q is 0: dd is finite
        ahead += (key > tkey || (key == tkey && idx < tidx)) ? 1u : 0u;
        if (key == maxkey) first = idx < first ? idx : first;
    };
    auto sweep = [&](int i) {
        u32 k[4];
        if constexpr (NCH > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) k[e] = kreg[NCH ? i : 0][e];
        } else {
            u32 f = 0u;
            load_chunk<BF16, GUIDED>(a, row, tid + NT * i, k, f);
        }
        const u32 i0 = 4u * (u32)(tid + NT * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            code(k[e], i0 + e);
            if (e & 1) __builtin_amdgcn_sched_barrier(0);         // two codes' masses and fp64 terms in flight, not 64: the keys hold 64 registers already
        }
    };
    if constexpr (NCH > 0) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) sweep(i);
    } else if (a.C >= 4) {
        for (int i = 0; i < n_it; ++i) sweep(i);
    }
    if (tid == 0) {
#pragma unroll
        for (int e = 0; e < 3; ++e) code(sh.ktail[e], tail0 + e);    // a key 0 (no such code) adds nothing
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        q_sum += shfl_xor_u64(q_sum, o);
        h_sum += shfl_xor_u64(h_sum, o);
        ahead += __shfl_xor(ahead, o, WAVE);
        const u32 f = __shfl_xor(first, o, WAVE);
        first = f < first ? f : first;
    }
    if (lane == 0) { atomicAdd(&sh.qtot, q_sum); atomicAdd(&sh.hsum, h_sum); atomicAdd(&sh.ahead, ahead); atomicMin(&sh.first, first); }
    __syncthreads();

    if (tid == 0) {
        const u64 q_total = sh.qtot;
        const double log_z = log((double)q_total * 2.3283064365386963e-10);       // Q_total * 2^-32 >= 1
        const double h = log_z + (double)sh.hsum / (65536.0 * (double)q_total);
        a.entropy[r] = (float)h;
        a.top_id[r] = (int)sh.first;
        a.mass[2 * (size_t)r] = q_total;
        if (scored) {
            const float lt = f32_from_orderable(tkey);
            a.logprob[r] = (float)(((double)lt - (double)m) - log_z);
            a.rank[r] = (int)sh.ahead;
            float dd;
            a.mass[2 * (size_t)r + 1] = mass_of(lt - m, dd);
        } else {
            a.logprob[r] = 0.0f;
            a.rank[r] = -1;
            a.mass[2 * (size_t)r + 1] = 0ull;
            atomicAdd(a.ignored, 1u);
        }
    }
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

int selftok_score_tokens(const void* logits, const void* uncond_logits, int dtype, int R, int C, long row_stride, long offset, float cfg_scale, float temperature,
                         const void* ids, int id_bytes, int rows_per_seq, long id_seq_stride, long id_step_stride, float* logprob, unsigned long long* mass,
                         int* rank, int* top_id, float* entropy, unsigned* bad, unsigned* ignored, hipStream_t stream)
{
    char msg[320];
    if (dtype != 0 && dtype != 1) {
        snprintf(msg, sizeof msg, "token_score: dtype must be 0 (fp32) or 1 (bf16), got %d", dtype); set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (id_bytes != 4 && id_bytes != 8) {
        snprintf(msg, sizeof msg, "token_score: id_bytes must be 4 (int32) or 8 (int64), got %d", id_bytes); set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (C < 1 || C > MAX_C) { snprintf(msg, sizeof msg, "token_score: need 1 <= C <= %d, got %d", MAX_C, C); set_last_error(msg); return SELFTOK_EINVAL; }
    if (R < 0 || offset < 0 || row_stride < 0 || offset > row_stride || (long)C > row_stride - offset) {
        snprintf(msg, sizeof msg, "token_score: need R >= 0 and the window [offset, offset + C) inside the row: R %d, offset %ld, C %d, row_stride %ld", R, offset, C,
                 row_stride);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (rows_per_seq < 1) {
        snprintf(msg, sizeof msg, "token_score: need rows_per_seq >= 1, got %d", rows_per_seq); set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (!(temperature > 0.0f) || isinf(temperature) || (uncond_logits && !(fabsf(cfg_scale) <= 3.0e38f))) {
        set_last_error("token_score: need a finite temperature > 0 (a greedy distribution has no log-probabilities) and a finite cfg_scale");
        return SELFTOK_EINVAL;
    }
    const float inv_T = 1.0f / temperature;
    if (isinf(inv_T)) { set_last_error("token_score: 1 / temperature is not finite"); return SELFTOK_EINVAL; }
    if (R == 0) return SELFTOK_OK;
    if (!logits || !ids || !logprob || !mass || !rank || !top_id || !entropy || !bad || !ignored) {
        set_last_error("token_score: null pointer"); return SELFTOK_EINVAL;
    }
    const uintptr_t row_align = dtype == 1 ? 8 : 16;              // four codes: one vector load
    if (((uintptr_t)logits % row_align) != 0 || ((uintptr_t)uncond_logits % row_align) != 0 || (offset & 3) != 0 || (R > 1 && (row_stride & 3) != 0)) {
        set_last_error("token_score: misaligned rows: the logits pointers must be aligned to four codes (16 bytes fp32, 8 bytes bf16), offset and row_stride "
                       "multiples of 4");
        return SELFTOK_EINVAL;
    }
    if (((uintptr_t)ids % (uintptr_t)id_bytes) != 0 || ((uintptr_t)logprob & 3) != 0 || ((uintptr_t)mass & 7) != 0 || ((uintptr_t)rank & 3) != 0 ||
        ((uintptr_t)top_id & 3) != 0 || ((uintptr_t)entropy & 3) != 0 || ((uintptr_t)bad & 3) != 0 || ((uintptr_t)ignored & 3) != 0) {
        set_last_error("token_score: logprob, rank, top_id, entropy, bad and ignored must be 4-byte aligned, mass 8-byte aligned, ids aligned to id_bytes");
        return SELFTOK_EINVAL;
    }
    ScoreArgs a;
    a.logits = logits; a.uncond = uncond_logits; a.ids = ids;
    a.logprob = logprob; a.mass = mass; a.rank = rank; a.top_id = top_id; a.entropy = entropy; a.bad = bad; a.ignored = ignored;
    a.row_stride = row_stride; a.offset = offset; a.id_seq_stride = id_seq_stride; a.id_step_stride = id_step_stride;
    a.R = R; a.C = C; a.id_bytes = id_bytes; a.S = rows_per_seq;
    a.cfg_scale = cfg_scale; a.inv_T = inv_T;
    const unsigned gx = R < GRID_X ? (unsigned)R : (unsigned)GRID_X;
    const dim3 grid(gx, (unsigned)(((long)R + GRID_X - 1) / GRID_X)), block(NT);
    const bool bf = dtype == 1, gd = uncond_logits != nullptr;
#define SCORE_LAUNCH(NCH)                                                                                                     \
    do {                                                                                                                      \
        if (bf && gd) hipLaunchKernelGGL((tok_score_kernel<NCH, true, true>), grid, block, 0, stream, a);                     \
        else if (bf) hipLaunchKernelGGL((tok_score_kernel<NCH, true, false>), grid, block, 0, stream, a);                     \
        else if (gd) hipLaunchKernelGGL((tok_score_kernel<NCH, false, true>), grid, block, 0, stream, a);                     \
        else hipLaunchKernelGGL((tok_score_kernel<NCH, false, false>), grid, block, 0, stream, a);                            \
    } while (0)
    if (C <= SMALL_CH * 4 * NT) SCORE_LAUNCH(SMALL_CH);
    else if (C <= REG_CH * 4 * NT) SCORE_LAUNCH(REG_CH);
    else SCORE_LAUNCH(0);
#undef SCORE_LAUNCH
    return check_launch("token_score kernel");
}

}  // extern "C"
