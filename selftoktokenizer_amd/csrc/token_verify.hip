// Speculative token sampling: verify S drafted ids per sequence against the target model's logits, on the sampler's arithmetic (include/selftok_hip_ext.h
// states the arithmetic of record; selftoktokenizer_amd/sampling.py is the host side; tests/token_spec_cases.py restates every step in numpy).
//
// tok_verify_kernel: a workgroup of 1024 threads owns one row (sequence b, draft slot s), grid B * (S + 1).  Both rows of logits -- the target's and the
// draft's -- are STREAMED: thread t owns the 4-code chunks t, t + 1024, .. and reads them again in every pass, served by the L2, exactly as the sampler does
// above 32768 codes.  No key lives in a register across passes and none in LDS, so one body serves either side, either dtype and every C up to 65536 at a
// fraction of the register file (DESIGN 37 has the reason).  Each side runs the sampler's steps: maximum, window mass, the top-k and top-p radix selects on the
// 48-bit order word (a cut is ONE number), then one sweep for the kept mass and count.  The accept test is an integer comparison of two 128-bit products; the
// residual weights are 128-bit differences shifted into uint64, drawn by the sampler's index-order select.  No floating point beyond the sampler's own.
// tok_commit_kernel: one thread per sequence turns the per-row verdicts into ids, log-probabilities and kept counts at their tokenizer positions and advances
// the step counter.  The leaf functions (key, mass, Philox) are token_shared.h's; the chunk load and the select are restated here on this file's argument block.
// No inline assembly, no scratch, no workspace, no state.
#include "common.h"
#include "selftok_hip_ext.h"
#include "token_shared.h"
#include <math.h>
#include <stdio.h>

namespace selftok {
namespace {

using namespace tokshared;

constexpr int NT = 1024;                                          // threads per row
constexpr int MAX_C = 65536;                                      // the index half of an order word is 16 bits
constexpr int MAX_S = 64;
constexpr int W_SHIFT = 34;                                       // residual weights: (p_i D - d_i P) >> 34 < 2^48, their sum < P D / 2^34 < 2^64

struct Side {
    const void* logits; const void* uncond;
    long seq_stride, row_stride;
    float cfg_scale;
};

struct VerifyArgs {
    Side t, d;
    const void* draft_ids; const int* n_draft; u32* ctr;
    unsigned char* accept; int* repl_id; int* n_kept; u64* mass; float* lp_x; float* lp_repl; u32* foreign; u32* bad;
    void* ids; float* lp_mat; int* nk_mat; int* n_accept; int* n_emit;
    long offset, draft_id_stride, id_row_stride, lp_row_stride, nk_row_stride;
    int B, S, C, K, draft_id_bytes, id_bytes, greedy, top_k;
    float inv_T, top_p;
    u32 seed_lo, seed_hi;
};

struct Shared {
    u64 hist[256];
    u64 part[NT / WAVE];
    u64 total, need, bin;
    u32 partc[NT / WAVE];
    u32 digit;
};

struct u128 { u64 hi, lo; };
__device__ __forceinline__ u128 mul64(u64 a, u64 b) { return {__umul64hi(a, b), a * b}; }
__device__ __forceinline__ bool less128(u128 a, u128 b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

// ---- block reductions through one slot per wave: integer, so any order gives the same bits ----
__device__ __forceinline__ u64 block_sum(Shared& sh, u64 v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += shfl_xor_u64(v, o);
    __syncthreads();                                              // the previous reduction's readers are done
    if ((threadIdx.x & 63) == 0) sh.part[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 s = 0ull;
#pragma unroll
    for (int w = 0; w < NT / WAVE; ++w) s += sh.part[w];
    return s;
}
template <bool MAX>
__device__ __forceinline__ u32 block_extreme(Shared& sh, u32 v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u32 w = __shfl_xor(v, o, WAVE); v = MAX ? (w > v ? w : v) : (w < v ? w : v); }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh.partc[threadIdx.x >> 6] = v;
    __syncthreads();
    u32 s = sh.partc[0];
#pragma unroll
    for (int w = 1; w < NT / WAVE; ++w) { const u32 x = sh.partc[w]; s = MAX ? (x > s ? x : s) : (x < s ? x : s); }
    return s;
}

template <bool BF16>
__device__ __forceinline__ float logit_at(const VerifyArgs& a, const Side& sd, size_t row, u32 idx)
{
    const bool guided = sd.uncond != nullptr;
    float lc, lu = 0.0f;
    if (BF16) {
        lc = widen(((const u16*)sd.logits)[row + idx]);
        if (guided) lu = widen(((const u16*)sd.uncond)[row + idx]);
    } else {
        lc = ((const float*)sd.logits)[row + idx];
        if (guided) lu = ((const float*)sd.uncond)[row + idx];
    }
    return scaled_logit(lc, lu, guided, sd.cfg_scale, a.inv_T);
}

// the keys of chunk j (codes 4 j .. 4 j + 3): one vector load per input when the chunk lies inside the window, code by code when it straddles its end; a code
// past the window gets key 0 and is skipped by its index everywhere
template <bool BF16>
__device__ __forceinline__ void load_chunk(const VerifyArgs& a, const Side& sd, size_t row, int j, u32 k[4], u32& badf)
{
    const u32 i0 = 4u * (u32)j;
    const bool guided = sd.uncond != nullptr;
    float lc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, lu[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i0 + 3u < (u32)a.C) {
        if (BF16) {
            const u16x4 v = *(const u16x4*)((const u16*)sd.logits + row + i0);
#pragma unroll
            for (int e = 0; e < 4; ++e) lc[e] = widen(v[e]);
            if (guided) {
                const u16x4 w = *(const u16x4*)((const u16*)sd.uncond + row + i0);
#pragma unroll
                for (int e = 0; e < 4; ++e) lu[e] = widen(w[e]);
            }
        } else {
            const f32x4 v = *(const f32x4*)((const float*)sd.logits + row + i0);
#pragma unroll
            for (int e = 0; e < 4; ++e) lc[e] = v[e];
            if (guided) {
                const f32x4 w = *(const f32x4*)((const float*)sd.uncond + row + i0);
#pragma unroll
                for (int e = 0; e < 4; ++e) lu[e] = w[e];
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i0 + e < (u32)a.C) {
                if (BF16) {
                    lc[e] = widen(((const u16*)sd.logits)[row + i0 + e]);
                    if (guided) lu[e] = widen(((const u16*)sd.uncond)[row + i0 + e]);
                } else {
                    lc[e] = ((const float*)sd.logits)[row + i0 + e];
                    if (guided) lu[e] = ((const float*)sd.uncond)[row + i0 + e];
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        u32 f = 0u;
        const u32 key = key_of(scaled_logit(lc[e], lu[e], guided, sd.cfg_scale, a.inv_T), f);
        const bool in = i0 + e < (u32)a.C;
        k[e] = in ? key : 0u;
        badf |= in ? f : 0u;
    }
}

// fn(key, index) for every code of the window, this thread's share
template <bool BF16, class Fn>
__device__ __forceinline__ void for_each_code(const VerifyArgs& a, const Side& sd, size_t row, Fn&& fn)
{
    const int n_it = (a.C + 4 * NT - 1) / (4 * NT);
    for (int i = 0; i < n_it; ++i) {
        u32 k[4], ignored = 0u;
        const int j = (int)threadIdx.x + NT * i;
        load_chunk<BF16>(a, sd, row, j, k, ignored);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4u * (u32)j + e < (u32)a.C) fn(k[e], 4u * (u32)j + (u32)e);
    }
}

__device__ __forceinline__ u64 order_word(u32 key, u32 idx) { return ((u64)(~key) << 16) | (u64)idx; }

enum { SEL_COUNT = 0, SEL_MASS = 1, SEL_DRAW = 2 };

// Wave 0 scans the 256 bins (lane L: bins 4 L .. 4 L + 3), clears them for the next pass and leaves the chosen digit, what is still needed inside it and the
// bin's content in sh.  On the first pass the need comes from the mode: the k of top-k, ceil(P * total), or mulhi64(u, total) + 1.  Called by every thread
// between two barriers of its own.
template <int MODE>
__device__ __forceinline__ void scan_bins(Shared& sh, bool first, u64 need0, float top_p, u64 u)
{
    const int tid = threadIdx.x, lane = tid & 63;
    __syncthreads();
    if (tid < WAVE) {
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
        u64 need = first ? need0 : sh.need;
        if (first && MODE == SEL_MASS) need = (u64)ceil((double)top_p * (double)tot);
        if (first && MODE == SEL_DRAW) need = __umul64hi(u, tot) + 1ull;              // running mass > r  <=>  running mass >= r + 1
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
            if (first) sh.total = tot;
        }
    }
    __syncthreads();
}

// The smallest order word whose inclusive prefix -- over the codes at or below cut_in, ascending -- reaches the need: SEL_COUNT counts codes (need the k of
// top-k), SEL_MASS sums integer masses (need ceil(P * the mass at or below cut_in)).  The sampler's select, 8 bits per pass from the top byte down.
template <int MODE, bool BF16>
__device__ __forceinline__ u64 select_cut(const VerifyArgs& a, const Side& sd, size_t row, Shared& sh, u64 cut_in, float m, u64 need0)
{
    u64 prefix = 0;
#pragma nounroll
    for (int s = 40; s >= 0; s -= 8) {
        u64 acc = 0;
        int cur = 0;
        for_each_code<BF16>(a, sd, row, [&](u32 key, u32 idx) {
            const u64 word = order_word(key, idx);
            if (word > cut_in) return;
            if (s != 40 && (word >> (s + 8)) != (prefix >> (s + 8))) return;
            const int dg = (int)((word >> s) & 255u);
            const u64 w = MODE == SEL_COUNT ? 1ull : mass_of(key, m);
            if (dg != cur) {                                      // runs of equal digits are merged before the histogram is touched
                if (acc) atomicAdd(&sh.hist[cur], acc);
                cur = dg; acc = 0;
            }
            acc += w;
        });
        if (acc) atomicAdd(&sh.hist[cur], acc);
        scan_bins<MODE>(sh, s == 40, need0, a.top_p, 0ull);
        prefix |= (u64)sh.digit << s;
        // the whole bin is wanted: every code under this prefix is kept.  Masses: only once the bin is inside one key (equal, positive masses) -- a wider bin
        // may end in codes of mass 0, which the shortest prefix leaves out.
        if ((MODE == SEL_COUNT || s <= 16) && sh.need == sh.bin) {
            prefix |= (1ull << s) - 1ull;
            break;
        }
    }
    return prefix;
}

// The sampler's index-order draw on integer weights: the first index whose running weight reaches mulhi64(u, total) + 1.  for_each_w(fn(index, weight)) walks
// this thread's codes; `total` returns the sum of all weights (0: nothing can be drawn, the returned index means nothing).
template <class ForEachW>
__device__ __forceinline__ u32 select_index(ForEachW&& for_each_w, Shared& sh, u64 u, u64& total)
{
    u32 prefix = 0u;
#pragma nounroll
    for (int s = 8; s >= 0; s -= 8) {
        u64 acc = 0;
        int cur = 0;
        for_each_w([&](u32 idx, u64 w) {
            if (w == 0ull) return;
            if (s != 8 && (idx >> 8) != (prefix >> 8)) return;
            const int dg = (int)((idx >> s) & 255u);
            if (dg != cur) {
                if (acc) atomicAdd(&sh.hist[cur], acc);
                cur = dg; acc = 0;
            }
            acc += w;
        });
        if (acc) atomicAdd(&sh.hist[cur], acc);
        scan_bins<SEL_DRAW>(sh, s == 8, 0ull, 0.0f, u);
        prefix |= sh.digit << s;
        if (s == 8) total = sh.total;
    }
    return prefix;
}

// what one side of a row comes to: steps 1 - 6 of the sampler's text
struct SideState {
    u32 maxkey, nkept;
    u64 cut, kept, qtot;                                          // the order word of the last kept code, Q_kept, Q_total
    bool bad;
};

template <bool BF16>
__device__ __forceinline__ SideState prepare(const VerifyArgs& a, const Side& sd, size_t row, Shared& sh)
{
    SideState st;
    u32 mx = 0u, badf = 0u;
    {
        const int n_it = (a.C + 4 * NT - 1) / (4 * NT);
        for (int i = 0; i < n_it; ++i) {
            u32 k[4];
            load_chunk<BF16>(a, sd, row, (int)threadIdx.x + NT * i, k, badf);
#pragma unroll
            for (int e = 0; e < 4; ++e) mx = k[e] > mx ? k[e] : mx;          // a code past the window has key 0: below every real key
        }
    }
    st.maxkey = block_extreme<true>(sh, mx);
    st.bad = block_extreme<true>(sh, badf) != 0u || st.maxkey <= KEY_NEG_INF;
    st.nkept = 0u; st.cut = ~0ull; st.kept = 0ull; st.qtot = 0ull;
    if (st.bad) return st;                                        // block-uniform
    const float m = f32_from_orderable(st.maxkey);
    const u32 maxkey = st.maxkey;

    u64 q = 0ull;
    u32 first = 0xFFFFFFFFu;
    for_each_code<BF16>(a, sd, row, [&](u32 key, u32 idx) {
        q += mass_of(key, m);
        if (key == maxkey) first = idx < first ? idx : first;
    });
    st.qtot = block_sum(sh, q);
    if (a.greedy) {
        st.cut = order_word(maxkey, block_extreme<false>(sh, first));          // the kept set is the first code of the order
    } else {
        if (a.top_k > 0) st.cut = select_cut<SEL_COUNT, BF16>(a, sd, row, sh, st.cut, m, (u64)a.top_k);
        if (a.top_p > 0.0f && a.top_p < 1.0f) st.cut = select_cut<SEL_MASS, BF16>(a, sd, row, sh, st.cut, m, 0ull);
    }
    const u64 cut = st.cut;
    u64 kq = 0ull, kn = 0ull;
    for_each_code<BF16>(a, sd, row, [&](u32 key, u32 idx) {
        if (order_word(key, idx) <= cut) { kq += mass_of(key, m); kn += 1ull; }
    });
    st.kept = block_sum(sh, kq);
    st.nkept = (u32)block_sum(sh, kn);
    return st;
}

// the mass of code idx inside a side's kept set, else 0
__device__ __forceinline__ u64 kept_mass(u32 key, u32 idx, u64 cut, float m) { return order_word(key, idx) <= cut ? mass_of(key, m) : 0ull; }

template <bool TB, bool DB>
__global__ void __launch_bounds__(NT) tok_verify_kernel(const VerifyArgs a)
{
    __shared__ Shared sh;
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (u32)(a.S + 1)), s = (int)(blockIdx.x % (u32)(a.S + 1));
    const size_t r = blockIdx.x;
    int nd = a.n_draft ? a.n_draft[b] : a.S;
    nd = nd < 0 ? 0 : (nd > a.S ? a.S : nd);
    long long x = -1;
    if (s < nd) {
        const size_t o = (size_t)b * (size_t)a.draft_id_stride + (size_t)s;
        x = a.draft_id_bytes == 8 ? ((const long long*)a.draft_ids)[o] : (long long)((const int*)a.draft_ids)[o];
        x = x < 0 ? -1 : x;
    }
    const bool has = x >= 0;                                      // block-uniform, as everything below that steers control flow
    const u32 ticket = a.ctr[2 * (size_t)b], step = a.ctr[2 * (size_t)b + 1] + (u32)s;
    const size_t trow = (size_t)b * (size_t)a.t.seq_stride + (size_t)s * (size_t)a.t.row_stride + (size_t)a.offset;
    const size_t drow = (size_t)b * (size_t)a.d.seq_stride + (size_t)s * (size_t)a.d.row_stride + (size_t)a.offset;       // only read when s < n_draft <= S

    if (tid < 256) sh.hist[tid] = 0ull;
    __syncthreads();

    const SideState T = prepare<TB>(a, a.t, trow, sh);
    bool bad = T.bad || x >= (long long)a.C;
    SideState D = T;
    if (has && !bad) {
        D = prepare<DB>(a, a.d, drow, sh);
        bad = D.bad;
    }
    const float qnan = __uint_as_float(0x7FC00000u);
    if (bad) {
        if (tid == 0) {
            a.accept[r] = 0; a.repl_id[r] = -1; a.n_kept[r] = 0;
            a.mass[4 * r] = 0ull; a.mass[4 * r + 1] = 0ull; a.mass[4 * r + 2] = 0ull; a.mass[4 * r + 3] = 0ull;
            a.lp_x[r] = qnan; a.lp_repl[r] = qnan;
            atomicAdd(a.bad, 1u);
        }
        return;
    }
    const float mt = f32_from_orderable(T.maxkey), md = f32_from_orderable(D.maxkey);
    const u64 P = T.kept, Dq = has ? D.kept : 0ull;

    // the draw from the target's own kept set: the sampler's step 7, counter word 2 = 0
    auto draw_target = [&](u64& total) {
        u32 o0, o1;
        philox4x32_10(ticket, step, 0u, 0u, a.seed_lo, a.seed_hi, o0, o1);
        return select_index([&](auto&& fn) {
            for_each_code<TB>(a, a.t, trow, [&](u32 key, u32 idx) { fn(idx, kept_mass(key, idx, T.cut, mt)); });
        }, sh, (u64)o0 | ((u64)o1 << 32), total);
    };

    u32 ignored = 0u;
    u64 p_x = 0ull, d_x = 0ull;
    u32 key_x = 0u;
    bool accept = false;
    if (has) {
        key_x = key_of(logit_at<TB>(a, a.t, trow, (u32)x), ignored);
        p_x = kept_mass(key_x, (u32)x, T.cut, mt);
        d_x = kept_mass(key_of(logit_at<DB>(a, a.d, drow, (u32)x), ignored), (u32)x, D.cut, md);
        u32 o0, o1;
        philox4x32_10(ticket, step, 1u, 0u, a.seed_lo, a.seed_hi, o0, o1);
        // u32 * d_x * P < p_x * D * 2^32, both sides below 2^114
        const u128 dp = mul64(d_x, P), lo = mul64(dp.lo, (u64)o0);
        const u128 lhs = {dp.hi * (u64)o0 + lo.hi, lo.lo};
        const u128 pd = mul64(p_x, Dq);
        const u128 rhs = {(pd.hi << 32) | (pd.lo >> 32), pd.lo << 32};
        accept = d_x > 0ull && less128(lhs, rhs);
    }

    u32 id = 0u;
    if (!accept) {                                                // block-uniform
        u64 total = 0ull;
        if (has) {
            u32 o0, o1;
            philox4x32_10(ticket, step, 2u, 0u, a.seed_lo, a.seed_hi, o0, o1);
            id = select_index([&](auto&& fn) {
                const int n_it = (a.C + 4 * NT - 1) / (4 * NT);
                for (int i = 0; i < n_it; ++i) {
                    u32 kt[4], kd[4], ign = 0u;
                    const int j = tid + NT * i;
                    load_chunk<TB>(a, a.t, trow, j, kt, ign);
                    load_chunk<DB>(a, a.d, drow, j, kd, ign);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const u32 idx = 4u * (u32)j + (u32)e;
                        if (idx >= (u32)a.C) continue;
                        const u128 pa = mul64(kept_mass(kt[e], idx, T.cut, mt), Dq), da = mul64(kept_mass(kd[e], idx, D.cut, md), P);
                        u64 w = 0ull;
                        if (less128(da, pa)) {
                            const u64 dl = pa.lo - da.lo, dh = pa.hi - da.hi - (pa.lo < da.lo ? 1ull : 0ull);
                            w = (dh << (64 - W_SHIFT)) | (dl >> W_SHIFT);
                        }
                        fn(idx, w);
                    }
                }
            }, sh, (u64)o0 | ((u64)o1 << 32), total);
        }
        if (total == 0ull) id = draw_target(total);              // no draft, or a residual that is zero everywhere
        id = id < (u32)a.C ? id : (u32)a.C - 1u;                    // the chosen code has positive weight, so it is a code of the window: this only fences the read below
    }

    if (tid == 0) {
        a.accept[r] = accept ? 1 : 0;
        a.n_kept[r] = (int)T.nkept;
        float lpx = qnan, lpr = qnan;
        const double log_q = log((double)T.qtot * 2.3283064365386963e-10);
        u64 m2 = p_x;
        if (has) lpx = (float)(((double)f32_from_orderable(key_x) - (double)mt) - log_q);
        if (!accept) {
            const u32 key = key_of(logit_at<TB>(a, a.t, trow, id), ignored);
            lpr = (float)(((double)f32_from_orderable(key) - (double)mt) - log_q);
            if (!has) m2 = mass_of(key, mt);                      // a row without a draft reports the mass of the code it drew, as the sampler does
        }
        a.repl_id[r] = accept ? -1 : (int)id;
        a.mass[4 * r] = P; a.mass[4 * r + 1] = Dq; a.mass[4 * r + 2] = m2; a.mass[4 * r + 3] = d_x;
        a.lp_x[r] = lpx; a.lp_repl[r] = lpr;
        if (has && d_x == 0ull) atomicAdd(a.foreign, 1u);
    }
}

// one thread per sequence: the accepted prefix, the replacement (or the bonus draw) after it, into tokenizer positions K - 1 - (step + j)
__global__ void __launch_bounds__(256) tok_commit_kernel(const VerifyArgs a)
{
    const int b = (int)(blockIdx.x * 256u + threadIdx.x);
    if (b >= a.B) return;
    int nd = a.n_draft ? a.n_draft[b] : a.S;
    nd = nd < 0 ? 0 : (nd > a.S ? a.S : nd);
    const size_t r0 = (size_t)b * (size_t)(a.S + 1);
    int na = 0;
    while (na < nd && a.accept[r0 + na]) ++na;
    const u32 step = a.ctr[2 * (size_t)b + 1];
    const int room = step < (u32)a.K ? a.K - (int)step : 0;
    const int ne = na + 1 < room ? na + 1 : room;
    for (int j = 0; j < ne; ++j) {
        const size_t r = r0 + (size_t)j;
        long long id;
        if (j < na) {
            const size_t o = (size_t)b * (size_t)a.draft_id_stride + (size_t)j;
            id = a.draft_id_bytes == 8 ? ((const long long*)a.draft_ids)[o] : (long long)((const int*)a.draft_ids)[o];
        } else {
            id = (long long)a.repl_id[r];
        }
        const size_t pos = (size_t)(a.K - 1 - ((int)step + j));
        const size_t o = (size_t)b * (size_t)a.id_row_stride + pos;
        if (a.id_bytes == 8) ((long long*)a.ids)[o] = id; else ((int*)a.ids)[o] = (int)id;
        a.lp_mat[(size_t)b * (size_t)a.lp_row_stride + pos] = j < na ? a.lp_x[r] : a.lp_repl[r];
        a.nk_mat[(size_t)b * (size_t)a.nk_row_stride + pos] = a.n_kept[r];
    }
    a.ctr[2 * (size_t)b + 1] = step + (u32)ne;
    a.n_accept[b] = na;
    a.n_emit[b] = ne;
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

int selftok_verify_draft(const void* target, const void* target_uncond, int target_dtype, long target_seq_stride, long target_row_stride, const void* draft,
                         const void* draft_uncond, int draft_dtype, long draft_seq_stride, long draft_row_stride, const void* draft_ids, int draft_id_bytes,
                         long draft_id_stride, const int* n_draft_host, const int* n_draft, int B, int S, int C, long offset, float cfg_scale,
                         float draft_cfg_scale, float temperature, int top_k, float top_p, unsigned seed_lo, unsigned seed_hi, unsigned* ctr,
                         unsigned char* accept, int* repl_id, int* n_kept, unsigned long long* mass, float* logprob_x, float* logprob_repl, void* ids,
                         int id_bytes, long id_row_stride, int K, float* logprob_out, long logprob_row_stride, int* n_kept_out, long n_kept_row_stride,
                         int* n_accept, int* n_emit, unsigned* foreign, unsigned* bad, hipStream_t stream)
{
    char msg[320];
    if ((target_dtype != 0 && target_dtype != 1) || (draft_dtype != 0 && draft_dtype != 1)) {
        snprintf(msg, sizeof msg, "verify_draft: each dtype must be 0 (fp32) or 1 (bf16), got target %d, draft %d", target_dtype, draft_dtype);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if ((id_bytes != 4 && id_bytes != 8) || (draft_id_bytes != 4 && draft_id_bytes != 8)) {
        snprintf(msg, sizeof msg, "verify_draft: id_bytes must be 4 (int32) or 8 (int64), got ids %d, draft ids %d", id_bytes, draft_id_bytes);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (C < 1 || C > MAX_C) { snprintf(msg, sizeof msg, "verify_draft: need 1 <= C <= %d, got %d", MAX_C, C); set_last_error(msg); return SELFTOK_EINVAL; }
    if (S < 0 || S > MAX_S) { snprintf(msg, sizeof msg, "verify_draft: need 0 <= S <= %d drafted tokens, got %d", MAX_S, S); set_last_error(msg); return SELFTOK_EINVAL; }
    if (B < 0 || (long)B * (long)(S + 1) >= (1l << 31) || offset < 0 || target_row_stride < 0 || target_seq_stride < 0 || offset > target_row_stride ||
        (long)C > target_row_stride - offset || (S > 0 && (draft_row_stride < 0 || draft_seq_stride < 0 || offset > draft_row_stride ||
                                                          (long)C > draft_row_stride - offset))) {
        snprintf(msg, sizeof msg, "verify_draft: need B >= 0 and the window [offset, offset + C) inside both rows: B %d, offset %ld, C %d, target row_stride %ld, "
                 "draft row_stride %ld", B, offset, C, target_row_stride, draft_row_stride);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (K < 1 || id_row_stride < 0 || logprob_row_stride < 0 || n_kept_row_stride < 0 || draft_id_stride < 0 ||
        (B > 1 && (id_row_stride < K || logprob_row_stride < K || n_kept_row_stride < K || draft_id_stride < S))) {
        snprintf(msg, sizeof msg, "verify_draft: need K >= 1, row strides of ids, logprob and n_kept >= K and of the draft ids >= S, got K %d, %ld, %ld, %ld, %ld", K,
                 id_row_stride, logprob_row_stride, n_kept_row_stride, draft_id_stride);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (!(temperature >= 0.0f) || isinf(temperature) || (target_uncond && !(fabsf(cfg_scale) <= 3.0e38f)) ||
        (draft_uncond && !(fabsf(draft_cfg_scale) <= 3.0e38f)) || top_p != top_p) {
        set_last_error("verify_draft: need a finite temperature >= 0 (0 = greedy), finite cfg scales and a top_p that is a number"); return SELFTOK_EINVAL;
    }
    const float inv_T = temperature == 0.0f ? 1.0f : 1.0f / temperature;
    if (isinf(inv_T)) { set_last_error("verify_draft: 1 / temperature is not finite"); return SELFTOK_EINVAL; }
    if ((n_draft_host == nullptr) != (n_draft == nullptr)) {
        set_last_error("verify_draft: n_draft_host (checked here) and n_draft (its device copy, read by the kernels) go together: pass both or neither");
        return SELFTOK_EINVAL;
    }
    if (n_draft_host)
        for (int b = 0; b < B; ++b)
            if (n_draft_host[b] < 0 || n_draft_host[b] > S) {
                snprintf(msg, sizeof msg, "verify_draft: need 0 <= n_draft[b] <= S = %d, got n_draft[%d] = %d", S, b, n_draft_host[b]);
                set_last_error(msg); return SELFTOK_EINVAL;
            }
    if (B == 0) return SELFTOK_OK;
    if (!target || (S > 0 && (!draft || !draft_ids)) || !ctr || !accept || !repl_id || !n_kept || !mass || !logprob_x || !logprob_repl || !ids || !logprob_out ||
        !n_kept_out || !n_accept || !n_emit || !foreign || !bad) {
        set_last_error("verify_draft: null pointer"); return SELFTOK_EINVAL;
    }
    const uintptr_t t_align = target_dtype == 1 ? 8 : 16, d_align = draft_dtype == 1 ? 8 : 16;           // four codes: one vector load
    if (((uintptr_t)target % t_align) != 0 || ((uintptr_t)target_uncond % t_align) != 0 || (offset & 3) != 0 || (target_row_stride & 3) != 0 ||
        (target_seq_stride & 3) != 0 || (S > 0 && (((uintptr_t)draft % d_align) != 0 || ((uintptr_t)draft_uncond % d_align) != 0 ||
                                                  (draft_row_stride & 3) != 0 || (draft_seq_stride & 3) != 0))) {
        set_last_error("verify_draft: misaligned rows: the logits pointers must be aligned to four codes of their dtype (16 bytes fp32, 8 bytes bf16), offset and "
                       "every row and sequence stride multiples of 4");
        return SELFTOK_EINVAL;
    }
    if (((uintptr_t)ctr & 3) != 0 || ((uintptr_t)n_draft & 3) != 0 || ((uintptr_t)draft_ids % (uintptr_t)draft_id_bytes) != 0 ||
        ((uintptr_t)ids % (uintptr_t)id_bytes) != 0 || ((uintptr_t)repl_id & 3) != 0 || ((uintptr_t)n_kept & 3) != 0 || ((uintptr_t)mass & 7) != 0 ||
        ((uintptr_t)logprob_x & 3) != 0 || ((uintptr_t)logprob_repl & 3) != 0 || ((uintptr_t)logprob_out & 3) != 0 || ((uintptr_t)n_kept_out & 3) != 0 ||
        ((uintptr_t)n_accept & 3) != 0 || ((uintptr_t)n_emit & 3) != 0 || ((uintptr_t)foreign & 3) != 0 || ((uintptr_t)bad & 3) != 0) {
        set_last_error("verify_draft: every 32-bit array must be 4-byte aligned, mass 8-byte aligned, ids and draft_ids aligned to their id_bytes");
        return SELFTOK_EINVAL;
    }
    VerifyArgs a;
    a.t = {target, target_uncond, target_seq_stride, target_row_stride, cfg_scale};
    a.d = {draft, draft_uncond, draft_seq_stride, draft_row_stride, draft_cfg_scale};
    a.draft_ids = draft_ids; a.n_draft = n_draft; a.ctr = ctr;
    a.accept = accept; a.repl_id = repl_id; a.n_kept = n_kept; a.mass = mass; a.lp_x = logprob_x; a.lp_repl = logprob_repl; a.foreign = foreign; a.bad = bad;
    a.ids = ids; a.lp_mat = logprob_out; a.nk_mat = n_kept_out; a.n_accept = n_accept; a.n_emit = n_emit;
    a.offset = offset; a.draft_id_stride = draft_id_stride; a.id_row_stride = id_row_stride; a.lp_row_stride = logprob_row_stride;
    a.nk_row_stride = n_kept_row_stride;
    a.B = B; a.S = S; a.C = C; a.K = K; a.draft_id_bytes = draft_id_bytes; a.id_bytes = id_bytes;
    a.greedy = temperature == 0.0f ? 1 : 0;
    a.top_k = a.greedy ? 1 : ((top_k <= 0 || top_k >= C) ? 0 : top_k);       // k >= C keeps every code: the same launch as top-k off
    a.top_p = a.greedy ? 1.0f : top_p;
    a.inv_T = inv_T;
    a.seed_lo = seed_lo; a.seed_hi = seed_hi;
    const dim3 grid((unsigned)(B * (S + 1))), block(NT);
    if (target_dtype == 1) {
        if (draft_dtype == 1) hipLaunchKernelGGL((tok_verify_kernel<true, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((tok_verify_kernel<true, false>), grid, block, 0, stream, a);
    } else {
        if (draft_dtype == 1) hipLaunchKernelGGL((tok_verify_kernel<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((tok_verify_kernel<false, false>), grid, block, 0, stream, a);
    }
    const int rc = check_launch("verify_draft verify kernel");
    if (rc != SELFTOK_OK) return rc;
    hipLaunchKernelGGL(tok_commit_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, a);
    return check_launch("verify_draft commit kernel");
}

}  // extern "C"
