// Token sampler: one row of AR logits over a window of C codes -> one code id (include/selftok_hip_ext.h states the arithmetic of record;
// selftoktokenizer_amd/sampling.py is the host side; tests/token_sample_cases.py restates every step in numpy).
//
// A workgroup of 1024 threads owns a row.  Thread t owns the 4-code chunks t, t + 1024, t + 2048, ..: one 16-byte load per chunk for fp32 logits, one 8-byte load
// for bf16; the chunk that straddles the end of the window is read code by code.  At C <= 32768 the row is read from memory ONCE and its 32 keys per thread stay
// in registers (tok_sample_kernel<8, .>); above that the chunks are read again in every pass (tok_sample_kernel<0, .>, the same arithmetic, served by the L2).
//
// Every code has the 48-bit ORDER WORD (~key) << 16 | index, key the monotone uint32 image of its fp32 logit (-0.0 counted as +0.0): ascending order words are the
// total order "logit descending, index ascending".  Both filters keep a prefix of that order, so each is ONE number, the order word of its last kept code, found by
// a radix select from the top byte down, 8 bits per pass, on a 256-bin LDS histogram of uint64 (counts for top-k, integer masses for top-p): the four key bytes
// find the pivot logit, the two index bytes cut its tie group by index.  A pass ends early when the whole bin is wanted (a tie group taken whole: the common
// case).  The draw is the same select on the 16 index bits alone over the kept codes: the first kept code in ascending index whose running mass exceeds r.
// Greedy rows run none of this: the lowest index at the maximum key falls out of the sweep that sums the window's mass.
// A thread merges runs of equal digits before it touches the histogram, integer adds commute: no sort, no workspace, no floating-point sum, the same bits for a
// row whatever shares its launch.  The only floating-point operations are the guidance / temperature products, the mass polynomial, one fp64 product and ceil for
// the top-p threshold and the fp64 log-probability.  No inline assembly, no scratch, no state.
#include "common.h"
#include "selftok_hip_ext.h"
#include "token_shared.h"
#include <math.h>
#include <stdio.h>

namespace selftok {
namespace {

using namespace tokshared;                                        // key, mass, Philox, shuffles: token_shared.h

constexpr int NT = 1024;                                          // threads per row
constexpr int REG_CH = 8;                                         // chunks of 4 codes a thread keeps in registers: 8 * 4 * 1024 = 32768
constexpr int MAX_C = 65536;                                      // the index half of an order word is 16 bits

struct SampleArgs {
    const void* logits; const void* uncond;
    const u32* ctr; const int* pos;
    void* ids_out; int* n_kept; u64* mass; float* logprob; u32* bad;
    long row_stride, offset, id_row_stride;
    int C, id_bytes, id_cols, greedy, top_k;
    float cfg_scale, inv_T, top_p;
    u32 seed_lo, seed_hi;
};

struct Shared {
    u64 hist[256];
    u64 total, need, bin, qtot;
    u32 digit, maxkey, flags, nkept, first;
    u32 zero;                                                     // always 0, read afresh in every pass: see for_each
};

template <bool BF16>
__device__ __forceinline__ float logit_at(const SampleArgs& a, size_t row, u32 idx)
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

// the keys of chunk j (codes 4 j .. 4 j + 3): one vector load per input when the chunk lies inside the window, code by code when it straddles its end; a code
// past the window gets key 0 and is skipped by its index everywhere
template <bool BF16>
__device__ __forceinline__ void load_chunk(const SampleArgs& a, size_t row, int j, u32 k[4], u32& badf)
{
    const u32 i0 = 4u * (u32)j;
    const bool guided = a.uncond != nullptr;
    float lc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, lu[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i0 + 3u < (u32)a.C) {
        if (BF16) {
            const u16x4 v = *(const u16x4*)((const u16*)a.logits + row + i0);
#pragma unroll
            for (int e = 0; e < 4; ++e) lc[e] = widen(v[e]);
            if (guided) {
                const u16x4 w = *(const u16x4*)((const u16*)a.uncond + row + i0);
#pragma unroll
                for (int e = 0; e < 4; ++e) lu[e] = widen(w[e]);
            }
        } else {
            const f32x4 v = *(const f32x4*)((const float*)a.logits + row + i0);
#pragma unroll
            for (int e = 0; e < 4; ++e) lc[e] = v[e];
            if (guided) {
                const f32x4 w = *(const f32x4*)((const float*)a.uncond + row + i0);
#pragma unroll
                for (int e = 0; e < 4; ++e) lu[e] = w[e];
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i0 + e < (u32)a.C) {
                if (BF16) {
                    lc[e] = widen(((const u16*)a.logits)[row + i0 + e]);
                    if (guided) lu[e] = widen(((const u16*)a.uncond)[row + i0 + e]);
                } else {
                    lc[e] = ((const float*)a.logits)[row + i0 + e];
                    if (guided) lu[e] = ((const float*)a.uncond)[row + i0 + e];
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        u32 f = 0u;
        const u32 key = key_of(scaled_logit(lc[e], lu[e], guided, a.cfg_scale, a.inv_T), f);
        const bool in = i0 + e < (u32)a.C;
        k[e] = in ? key : 0u;
        badf |= in ? f : 0u;
    }
}

enum { SEL_COUNT = 0, SEL_MASS = 1, SEL_DRAW = 2 };

// The smallest order word (SEL_DRAW: index) whose inclusive prefix -- over the codes at or below cut_in, in ascending order -- reaches `need`:
//   SEL_COUNT  prefix = number of codes, need = need0 (the k of top-k)
//   SEL_MASS   prefix = integer mass, need = ceil(P * total) of the first pass's total (the mass of the top-k prefix)
//   SEL_DRAW   prefix = integer mass in INDEX order, need = mulhi64(u, total) + 1; counts the kept codes on the way
// Block-uniform control flow throughout; `total` returns the first pass's total.
template <int MODE, class ForEach>
__device__ __forceinline__ u64 radix_select(ForEach& for_each, Shared& sh, const SampleArgs& a, int b, u64 cut_in, float m, u64 need0, u64& total)
{
    const int tid = threadIdx.x, lane = tid & 63;
    constexpr int TOP = MODE == SEL_DRAW ? 8 : 40;
    u64 prefix = 0;
#pragma nounroll
    for (int s = TOP; s >= 0; s -= 8) {
        u64 acc = 0;
        int cur = 0;
        u32 cnt = 0;
        for_each([&](u32 key, u32 idx) {
            const u64 word = ((u64)(~key) << 16) | (u64)idx;
            if (word > cut_in) return;
            const u64 c = MODE == SEL_DRAW ? (u64)idx : word;
            if (s != TOP && (c >> (s + 8)) != (prefix >> (s + 8))) return;
            const int dg = (int)((c >> s) & 255u);
            const u64 w = MODE == SEL_COUNT ? 1ull : mass_of(key, m);
            if (MODE == SEL_DRAW && s == TOP) cnt += 1u;
            if (dg != cur) {
                if (acc) atomicAdd(&sh.hist[cur], acc);
                cur = dg; acc = 0;
            }
            acc += w;
        });
        if (acc) atomicAdd(&sh.hist[cur], acc);
        if (MODE == SEL_DRAW && s == TOP) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, WAVE);
            if (lane == 0 && cnt) atomicAdd(&sh.nkept, cnt);
        }
        __syncthreads();
        if (tid < WAVE) {                                         // wave 0: lane L scans bins 4 L .. 4 L + 3 and clears them for the next pass
            u64 bin[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { bin[j] = sh.hist[4 * lane + j]; sh.hist[4 * lane + j] = 0ull; }
            const u64 own = (bin[0] + bin[1]) + (bin[2] + bin[3]);
            u64 incl = own;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const u64 v = shfl_up_u64(incl, o);
                if (lane >= o) incl += v;
            }
            const u64 tot = shfl_u64(incl, WAVE - 1);
            u64 need = s == TOP ? need0 : sh.need;
            if (s == TOP && MODE == SEL_MASS) need = (u64)ceil((double)a.top_p * (double)tot);
            if (s == TOP && MODE == SEL_DRAW) {
                u32 o0, o1;
                philox4x32_10(a.ctr[2 * (size_t)b], a.ctr[2 * (size_t)b + 1], 0u, 0u, a.seed_lo, a.seed_hi, o0, o1);
                need = __umul64hi((u64)o0 | ((u64)o1 << 32), tot) + 1ull;            // running mass > r  <=>  running mass >= r + 1
            }
            const u64 ball = __ballot(incl >= need);
            const int lf = ball ? __ffsll((unsigned long long)ball) - 1 : WAVE - 1;
            if (lane == lf) {
                u64 below = incl - own;
                int j = 0;
#pragma unroll
                for (int t = 0; t < 3; ++t)
                    if (j == t && below + bin[t] < need) { below += bin[t]; j = t + 1; }
                const u64 chosen = j == 0 ? bin[0] : (j == 1 ? bin[1] : (j == 2 ? bin[2] : bin[3]));
                sh.digit = (u32)(4 * lane + j);
                sh.need = need - below;
                sh.bin = chosen;
                if (s == TOP) sh.total = tot;
            }
        }
        __syncthreads();
        prefix |= (u64)sh.digit << s;
        if (s == TOP) total = sh.total;
        // the whole bin is wanted: every code under this prefix is kept.  Masses: only once the bin is inside one key (equal, positive masses) --
        // a wider bin may end in codes of mass 0, which the shortest prefix leaves out.
        if ((MODE == SEL_COUNT || (MODE == SEL_MASS && s <= 16)) && sh.need == sh.bin) {
            prefix |= (1ull << s) - 1ull;
            break;
        }
    }
    return prefix;
}

template <int NCH, bool BF16>
__global__ void __launch_bounds__(NT) tok_sample_kernel(const SampleArgs a)
{
    __shared__ Shared sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const size_t row = (size_t)b * (size_t)a.row_stride + (size_t)a.offset;
    const int n_it = NCH ? NCH : (a.C + 4 * NT - 1) / (4 * NT);

    if (tid < 256) sh.hist[tid] = 0ull;
    if (tid == 0) { sh.maxkey = 0u; sh.flags = 0u; sh.nkept = 0u; sh.qtot = 0ull; sh.zero = 0u; sh.first = 0xFFFFFFFFu; }
    __syncthreads();

    // ---- the one read of the row: keys, maximum, NaN / +inf ----
    u32 kreg[NCH ? NCH : 1][4];
    u32 mx = 0u, badf = 0u;
    auto first_read = [&](int i) {
        u32 k[4];
        load_chunk<BF16>(a, row, tid + NT * i, k, badf);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (NCH) kreg[NCH ? i : 0][e] = k[e];
            mx = k[e] > mx ? k[e] : mx;                           // a code past the window has key 0: below every real key
        }
    };
    if constexpr (NCH > 0) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) first_read(i);
    } else {
        for (int i = 0; i < n_it; ++i) first_read(i);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u32 v = __shfl_xor(mx, o, WAVE); mx = v > mx ? v : mx; }
    if (lane == 0) atomicMax(&sh.maxkey, mx);
    if (__ballot(badf != 0u) != 0ull && lane == 0) atomicOr(&sh.flags, 1u);
    __syncthreads();

    const int p = a.pos ? a.pos[b] : 0;
    const u32 maxkey = sh.maxkey;
    if (sh.flags != 0u || maxkey <= KEY_NEG_INF || p < 0 || p >= a.id_cols) {          // a bad row: block-uniform
        if (tid == 0) {
            if (p >= 0 && p < a.id_cols) {
                const size_t o = (size_t)b * (size_t)a.id_row_stride + (size_t)p;
                if (a.id_bytes == 8) ((long long*)a.ids_out)[o] = -1ll; else ((int*)a.ids_out)[o] = -1;
            }
            a.n_kept[b] = 0;
            a.mass[3 * (size_t)b] = 0ull; a.mass[3 * (size_t)b + 1] = 0ull; a.mass[3 * (size_t)b + 2] = 0ull;
            a.logprob[b] = __uint_as_float(0x7FC00000u);
            atomicAdd(a.bad, 1u);
        }
        return;
    }
    const float m = f32_from_orderable(maxkey);

    // The keys never change, so every pass's per-code work (order words, masses) is loop-invariant and the compiler would hoist all 32 codes' worth of it out of
    // the pass loop, far beyond the 128 registers a 1024-thread workgroup has.  XOR-ing the keys with a zero that is read afresh (volatile) per pass keeps the
    // work inside the pass: one VALU operation per code.
    auto for_each = [&](auto&& fn) {
        const u32 z = *(volatile u32*)&sh.zero;
        const u32 t4 = (4u * (u32)tid) ^ z;                       // the indices likewise: 32 of them hoisted would be 32 registers
        auto chunk = [&](int i) {
            u32 k[4];
            if constexpr (NCH > 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) k[e] = kreg[NCH ? i : 0][e];
            } else {
                u32 ignored = 0u;
                load_chunk<BF16>(a, row, tid + NT * i, k, ignored);
            }
            const u32 i0 = t4 + 4u * (u32)(NT * i);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < (u32)a.C) fn(k[e] ^ z, i0 + e);
            __builtin_amdgcn_sched_barrier(0);                    // one chunk at a time: 32 masses in flight would not fit the 128 registers of a 1024-thread workgroup
        };
        if constexpr (NCH > 0) {
#pragma unroll
            for (int i = 0; i < NCH; ++i) chunk(i);
        } else {
            for (int i = 0; i < n_it; ++i) chunk(i);
        }
    };

    // ---- the mass of the whole window (the log-probability's denominator); greedy: the first code of the order is the lowest index at the maximum key ----
    {
        u64 q = 0ull;
        u32 first = 0xFFFFFFFFu;
        for_each([&](u32 key, u32 idx) {
            q += mass_of(key, m);
            if (key == maxkey) first = idx < first ? idx : first;
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            q += shfl_xor_u64(q, o);
            const u32 f = __shfl_xor(first, o, WAVE);
            first = f < first ? f : first;
        }
        if (lane == 0) { atomicAdd(&sh.qtot, q); if (a.greedy) atomicMin(&sh.first, first); }
    }

    // ---- the two filters, then the draw ----
    u64 cut = ~0ull, total = 0ull;
    u32 id;
    if (a.greedy) {
        __syncthreads();
        id = sh.first;
        total = 1ull << 32;                                       // the mass of the maximum, exactly
        if (tid == 0) sh.nkept = 1u;
    } else {
        if (a.top_k > 0) cut = radix_select<SEL_COUNT>(for_each, sh, a, b, cut, m, (u64)a.top_k, total);
        if (a.top_p > 0.0f && a.top_p < 1.0f) cut = radix_select<SEL_MASS>(for_each, sh, a, b, cut, m, 0ull, total);
        id = (u32)radix_select<SEL_DRAW>(for_each, sh, a, b, cut, m, 0ull, total);
    }
    id = id < (u32)a.C ? id : (u32)a.C - 1u;                        // the chosen code has positive mass, so it is a code of the window: this only fences the read below

    if (tid == 0) {
        u32 ignored = 0u;
        const u32 key = key_of(logit_at<BF16>(a, row, id), ignored);
        const u64 q_total = sh.qtot;
        const size_t o = (size_t)b * (size_t)a.id_row_stride + (size_t)p;
        if (a.id_bytes == 8) ((long long*)a.ids_out)[o] = (long long)id; else ((int*)a.ids_out)[o] = (int)id;
        a.n_kept[b] = (int)sh.nkept;
        a.mass[3 * (size_t)b] = q_total; a.mass[3 * (size_t)b + 1] = total; a.mass[3 * (size_t)b + 2] = mass_of(key, m);
        const double lp = ((double)f32_from_orderable(key) - (double)m) - log((double)q_total * 2.3283064365386963e-10);
        a.logprob[b] = (float)lp;
    }
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

int selftok_sample_token(const void* logits, const void* uncond_logits, int dtype, int B, int C, long row_stride, long offset, float cfg_scale, float temperature,
                         int top_k, float top_p, unsigned seed_lo, unsigned seed_hi, const unsigned* ctr, const int* pos, void* ids_out, int id_bytes,
                         long id_row_stride, int id_cols, int* n_kept, unsigned long long* mass, float* logprob, unsigned* bad, hipStream_t stream)
{
    char msg[320];
    if (dtype != 0 && dtype != 1) {
        snprintf(msg, sizeof msg, "token_sample: dtype must be 0 (fp32) or 1 (bf16), got %d", dtype); set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (id_bytes != 4 && id_bytes != 8) {
        snprintf(msg, sizeof msg, "token_sample: id_bytes must be 4 (int32) or 8 (int64), got %d", id_bytes); set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (C < 1 || C > MAX_C) { snprintf(msg, sizeof msg, "token_sample: need 1 <= C <= %d, got %d", MAX_C, C); set_last_error(msg); return SELFTOK_EINVAL; }
    if (B < 0 || offset < 0 || row_stride < 0 || offset > row_stride || (long)C > row_stride - offset) {
        snprintf(msg, sizeof msg, "token_sample: need B >= 0 and the window [offset, offset + C) inside the row: B %d, offset %ld, C %d, row_stride %ld", B, offset, C,
                 row_stride);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (id_cols < 1 || id_row_stride < 0 || (pos == nullptr && B > 1 && id_row_stride < 1)) {
        snprintf(msg, sizeof msg, "token_sample: need id_cols >= 1 and id_row_stride >= 0 (>= 1 for several rows), got %d, %ld", id_cols, id_row_stride);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (!(temperature >= 0.0f) || isinf(temperature) || (uncond_logits && !(fabsf(cfg_scale) <= 3.0e38f)) || top_p != top_p) {
        set_last_error("token_sample: need a finite temperature >= 0 (0 = greedy), a finite cfg_scale and a top_p that is a number"); return SELFTOK_EINVAL;
    }
    const float inv_T = temperature == 0.0f ? 1.0f : 1.0f / temperature;
    if (isinf(inv_T)) { set_last_error("token_sample: 1 / temperature is not finite"); return SELFTOK_EINVAL; }
    if (B == 0) return SELFTOK_OK;
    if (!logits || !ctr || !ids_out || !n_kept || !mass || !logprob || !bad) { set_last_error("token_sample: null pointer"); return SELFTOK_EINVAL; }
    const uintptr_t row_align = dtype == 1 ? 8 : 16;              // four codes: one vector load
    if (((uintptr_t)logits % row_align) != 0 || ((uintptr_t)uncond_logits % row_align) != 0 || (offset & 3) != 0 || (B > 1 && (row_stride & 3) != 0)) {
        set_last_error("token_sample: misaligned rows: the logits pointers must be aligned to four codes (16 bytes fp32, 8 bytes bf16), offset and row_stride "
                       "multiples of 4");
        return SELFTOK_EINVAL;
    }
    if (((uintptr_t)ctr & 3) != 0 || ((uintptr_t)pos & 3) != 0 || ((uintptr_t)ids_out % (uintptr_t)id_bytes) != 0 || ((uintptr_t)n_kept & 3) != 0 ||
        ((uintptr_t)mass & 7) != 0 || ((uintptr_t)logprob & 3) != 0 || ((uintptr_t)bad & 3) != 0) {
        set_last_error("token_sample: ctr, pos, n_kept, logprob and bad must be 4-byte aligned, mass 8-byte aligned, ids_out aligned to id_bytes");
        return SELFTOK_EINVAL;
    }
    SampleArgs a;
    a.logits = logits; a.uncond = uncond_logits; a.ctr = ctr; a.pos = pos;
    a.ids_out = ids_out; a.n_kept = n_kept; a.mass = mass; a.logprob = logprob; a.bad = bad;
    a.row_stride = row_stride; a.offset = offset; a.id_row_stride = id_row_stride;
    a.C = C; a.id_bytes = id_bytes; a.id_cols = id_cols;
    a.greedy = temperature == 0.0f ? 1 : 0;
    a.top_k = a.greedy ? 1 : ((top_k <= 0 || top_k >= C) ? 0 : top_k);       // k >= C keeps every code: the same launch as top-k off
    a.top_p = a.greedy ? 1.0f : top_p;
    a.cfg_scale = cfg_scale; a.inv_T = inv_T;
    a.seed_lo = seed_lo; a.seed_hi = seed_hi;
    const dim3 grid((unsigned)B), block(NT);
    if (C <= REG_CH * 4 * NT) {
        if (dtype == 1) hipLaunchKernelGGL((tok_sample_kernel<REG_CH, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((tok_sample_kernel<REG_CH, false>), grid, block, 0, stream, a);
    } else {
        if (dtype == 1) hipLaunchKernelGGL((tok_sample_kernel<0, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((tok_sample_kernel<0, false>), grid, block, 0, stream, a);
    }
    return check_launch("token_sample kernel");
}

}  // extern "C"
