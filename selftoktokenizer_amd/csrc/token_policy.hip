// Token policy loss: one row of AR logits over a window of C codes, ONE SAMPLED id, the log-probability the id had when it was drawn and its advantage ->
// the clipped importance-ratio surrogate of PPO / GRPO, the k3 estimate of the KL to a frozen reference, the row's entropy, and the whole gradient row of
// g (-surrogate + kl_coef kl - ent_coef H), written over V columns and, if the caller says so, over the logits themselves (include/selftok_hip_ext.h states
// the arithmetic of record; selftoktokenizer_amd/losses.py is the host side; tests/token_policy_cases.py restates every step in numpy).
//
// The loss's shape (csrc/token_xent.hip): a workgroup of 512 threads owns a row, the grid is one workgroup per row (x = min(R, 65536), y the rest).  Thread t
// owns the 4-code chunks t, t + 512, ..: one 16-byte load and one 16-byte store per chunk for fp32, 8 bytes for bf16; the up to three codes of the partial
// chunk at the window's end are thread 0's, code by code, their keys parked in LDS.  Three sweeps: (1) keys, the maximum, NaN / +inf; (2) the integer mass q of
// every code, their sum Q and -- in the ENT instances -- the integer entropy sum S; (3) p = q / Q, the gradient, the store.  At C <= 32768 the row is read
// from memory ONCE (<16, ., false>; <2, ., .> for C <= 4096; <8, ., true> for C <= 16384 with the entropy sum): the keys stay in registers.  Above that (<0, ., .>) sweeps (2) and (3) read the chunks again through
// the L2.  Between (2) and (3) thread 0 takes the row's transcendentals -- one fp64 log, one exp, one expm1 -- and parks the three numbers sweep (3) needs
// (k, kH, E) in LDS.
//
// ENT, the one template parameter the loss kernel does not have: true when ent_coef != 0 OR the entropy output is requested.  Only these instances form S in
// sweep (2), and only they keep the KEYS in registers through sweep (3), which needs d_i = l_i - m beside q_i and computes the mass a second time; the
// others put the mass where the key was, as the loss kernel does, and run its sweep (3) instruction for instruction.  Whether the entropy term is ADDED to
// the gradient is decided by ent_coef != 0 alone, block-uniformly: with ent_coef == 0 the addition is not performed and the bits are the loss kernel's.
//
// In place (grad == logits) is correct for the loss kernel's two reasons.  (i) A thread stores only chunks it has itself loaded in its last sweep -- the
// partial chunk's codes are thread 0's in every sweep -- so no thread ever reads a code another thread may already have overwritten; a chunk past the window
// re-reads chunk 0, possibly overwritten by then, and masks what it read to nothing.  (ii) Nothing is stored before the barrier that completes Q (and S):
// every value that crosses threads -- the maximum, the flags, Q, S -- is final before the first store (the target's logit is read by every thread before the
// barrier that ends sweep (1), ahead of the zeros a bad row stores right after it), and the one barrier after it
// (k, kH, E) carries nothing that was read from the row after that point.  The zero rows of a bad or ignored row are stored after every read of that row.
// Every reduction is a maximum, an OR or an integer sum: any order gives the same bits.  No inline assembly, no scratch, no state, no workspace.
#include "common.h"
#include "selftok_hip_ext.h"
#include "token_shared.h"
#include <math.h>
#include <stdio.h>

namespace selftok {
namespace {

using namespace tokshared;

constexpr int NT = 512;                                           // threads per row
constexpr int REG_CH = 16;                                        // chunks of 4 codes a thread keeps in registers: 16 * 4 * 512 = 32768
constexpr int ENT_CH = 8;                                         // ... in the instances that form the entropy sum and keep the keys: 8 * 4 * 512 = 16384
constexpr int SMALL_CH = 2;                                       // 2 * 4 * 512 = 4096
constexpr int MAX_C = 65536;
constexpr int GRID_X = 65536;                                     // rows per grid row
constexpr u32 Q_ONE = 0xFFFFFFFFu;                                // the 32-bit image of the mass 2^32 (a mass is a multiple of 256 from 2^31 on)
constexpr u32 NAN_BITS = 0x7FC00000u;

struct PolicyArgs {
    const void* logits; const void* ids; const float* row_scale; const float* old_lp; const float* adv; const float* ref_lp; void* grad;
    float* logprob; float* lse; float* ratio; float* kl; float* entropy; float* coef; unsigned char* flags; u32* bad; u32* ignored;
    long row_stride, offset, id_seq_stride, id_step_stride, grad_stride, V;
    int R, C, id_bytes, S;
    float clip_lo, clip_hi, kl_coef, ent_coef;
};

struct Shared {
    u64 qtot, hsum;
    double E;
    u32 maxkey, flags;
    float k, kH;
    u32 ktail[3];                                                 // the keys of the partial chunk's up to three codes (0: no such code)
};

// fp32 -> bf16, to nearest even, once; a NaN stays one
__device__ __forceinline__ u16 narrow(float f)
{
    const u32 u = __float_as_uint(f);
    const u32 r = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    return (u & 0x7FFFFFFFu) > 0x7F800000u ? (u16)0x7FC0u : (u16)r;
}

__device__ __forceinline__ u32 mass32(u64 q) { return q > (u64)Q_ONE ? Q_ONE : (u32)q; }
__device__ __forceinline__ double mass_f64(u32 q32) { return q32 == Q_ONE ? 4294967296.0 : (double)q32; }

template <bool BF16>
__device__ __forceinline__ float logit_at(const PolicyArgs& a, size_t row, u32 idx)
{
    return BF16 ? widen(((const u16*)a.logits)[row + idx]) : ((const float*)a.logits)[row + idx];
}

template <bool BF16>
__device__ __forceinline__ void store_one(const PolicyArgs& a, size_t at, float v)
{
    if (BF16) ((u16*)a.grad)[at] = narrow(v);
    else ((float*)a.grad)[at] = v;
}

template <bool BF16>
__device__ __forceinline__ void store_four(const PolicyArgs& a, size_t at, const float v[4])
{
    if (BF16) {
        u16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = narrow(v[e]);
        *(u16x4*)((u16*)a.grad + at) = o;
    } else {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[e];
        *(f32x4*)((float*)a.grad + at) = o;
    }
}

// columns [lo, hi) of the gradient row at element `base` (a multiple of four) := +0: the codes up to the first multiple of four and past the last one by
// one thread each, whole chunks in between by vector stores
template <bool BF16>
__device__ __forceinline__ void zero_columns(const PolicyArgs& a, size_t base, long lo, long hi, int tid)
{
    if (lo >= hi) return;
    long a4 = (lo + 3) & ~3L;
    if (a4 > hi) a4 = hi;
    long b4 = hi & ~3L;
    if (b4 < a4) b4 = a4;
    const float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if ((long)tid < a4 - lo) store_one<BF16>(a, base + (size_t)(lo + tid), 0.0f);
    for (long c = a4 + 4L * tid; c < b4; c += 4L * NT) store_four<BF16>(a, base + (size_t)c, z);
    if ((long)tid < hi - b4) store_one<BF16>(a, base + (size_t)(b4 + tid), 0.0f);
}

// the keys of the whole chunk j (codes 4 j .. 4 j + 3 < C): one vector load; a chunk at or past the window's last, partial chunk reads chunk 0 instead (the
// caller has checked C >= 4) and gets keys 0 -- below every real key, a key 0 decodes to a NaN whose mass is 0 -- so that the chunks of a thread are one
// basic block
template <bool BF16>
__device__ __forceinline__ void load_chunk(const PolicyArgs& a, size_t row, int j, u32 k[4], u32& badf)
{
    const u32 i0 = 4u * (u32)j;
    const u32 in = (u32)((int)(i0 + 3u - (u32)a.C) >> 31);        // all ones inside the window; a vector mask
    const size_t at = row + (i0 & in);
    float l[4];
    if (BF16) {
        const u16x4 v = *(const u16x4*)((const u16*)a.logits + at);
#pragma unroll
        for (int e = 0; e < 4; ++e) l[e] = widen(v[e]);
    } else {
        const f32x4 v = *(const f32x4*)((const float*)a.logits + at);
#pragma unroll
        for (int e = 0; e < 4; ++e) l[e] = v[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        u32 f = 0u;
        const u32 key = key_of(l[e], f);
        k[e] = key & in;
        badf |= f & in;
    }
}

__device__ __forceinline__ float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ bool nan_or_pinf(float v) { return !(v < __uint_as_float(0x7F800000u)); }

template <int NCH, bool BF16, bool ENT>
__global__ void __launch_bounds__(NT, 4) tok_policy_kernel(const PolicyArgs a)
{
    __shared__ Shared sh;
    const long r = (long)blockIdx.y * GRID_X + (long)blockIdx.x;
    if (r >= (long)a.R) return;                                   // the last grid row: block-uniform
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t row = (size_t)r * (size_t)a.row_stride + (size_t)a.offset;
    const size_t grow = (size_t)r * (size_t)a.grad_stride;        // the gradient row's column 0
    const int n_it = NCH ? NCH : (a.C + 4 * NT - 1) / (4 * NT);
    const u32 tail0 = (u32)a.C & ~3u;                             // the first code of the partial chunk
    const bool want_grad = a.grad != nullptr;                     // block-uniform

    if (tid == 0) { sh.qtot = 0ull; sh.hsum = 0ull; sh.E = 0.0; sh.maxkey = 0u; sh.flags = 0u; sh.k = 0.0f; sh.kH = 0.0f; sh.ktail[0] = 0u; sh.ktail[1] = 0u; sh.ktail[2] = 0u; }

    // the target: every thread reads the same element
    const long io = (r / a.S) * a.id_seq_stride + (r % a.S) * a.id_step_stride;
    const long long tv_v = a.id_bytes == 8 ? ((const long long*)a.ids)[io] : (long long)((const int*)a.ids)[io];
    const long long tv = (long long)(((u64)(u32)__builtin_amdgcn_readfirstlane((int)((u64)tv_v >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)tv_v));
    // the target's key, read by every thread BEFORE the barrier that ends sweep 1: the row's kind below depends on it (-inf against -inf), and a bad row's zeros
    // are stored right after that barrier -- in place over the very element read here
    u32 tkey = 0u;
    if (tv >= 0 && tv < (long long)a.C) { u32 f = 0u; tkey = (u32)__builtin_amdgcn_readfirstlane((int)key_of(logit_at<BF16>(a, row, (u32)tv), f)); }
    __syncthreads();

    // ---- sweep 1, the one read of the row at C <= 32768: keys, maximum, NaN / +inf ----
    u32 kreg[NCH ? NCH : 1][4];
    u32 mx = 0u, badf = 0u;
    auto first_read = [&](int i) {
        u32 k[4];
        load_chunk<BF16>(a, row, tid + NT * i, k, badf);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (NCH) kreg[NCH ? i : 0][e] = k[e];
            mx = k[e] > mx ? k[e] : mx;
        }
        if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // four chunks' loads in flight per thread, not all sixteen
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

    // the row's kind, block-uniform: every thread reads the same scalars.  The operands of an IGNORED row (target < 0) are not looked at.
    const u32 maxkey = (u32)__builtin_amdgcn_readfirstlane((int)sh.maxkey);
    const bool scored = tv >= 0;
    bool is_bad = sh.flags != 0u || maxkey <= KEY_NEG_INF || tv >= (long long)a.C;
    const u32 tidx = (scored && !is_bad) ? (u32)tv : 0xFFFFFFFFu; // no code has this index
    float adv = 0.0f, old_lp = 0.0f, ref_lp = 0.0f;
    if (scored && !is_bad) {
        adv = uniform(a.adv[r]);                                  // block-uniform values belong in scalar registers
        old_lp = uniform(a.old_lp[r]);
        if (a.ref_lp) ref_lp = uniform(a.ref_lp[r]);
        const bool lp_ninf = tkey == KEY_NEG_INF;                 // the target's logit is -inf: so is its log-probability, and -inf minus -inf is a NaN
        is_bad = !(fabsf(adv) < __uint_as_float(0x7F800000u)) || nan_or_pinf(old_lp) || nan_or_pinf(ref_lp) ||
                 (lp_ninf && (old_lp == -__uint_as_float(0x7F800000u) || (a.ref_lp && ref_lp == -__uint_as_float(0x7F800000u))));
    }
    if (is_bad) {                                                 // every read of the row, the target's logit included, lies before the barrier above
        if (want_grad) zero_columns<BF16>(a, grow, 0L, a.V, tid);
        if (tid == 0) {
            const float nan = __uint_as_float(NAN_BITS);
            a.logprob[r] = nan; a.lse[r] = nan; a.ratio[r] = nan; a.kl[r] = nan; a.coef[r] = nan;
            if (a.entropy) a.entropy[r] = nan;
            a.flags[r] = 0;
            atomicAdd(a.bad, 1u);
        }
        return;
    }
    const float m = f32_from_orderable(maxkey);

    // ---- sweep 2: the integer masses, their sum and (ENT) the integer entropy sum ----
    u64 q_sum = 0ull, h_sum = 0ull;
    auto code = [&](u32 key) {
        const u64 q = mass_of(key, m);
        const u32 q32 = mass32(q);
        q_sum += q32 == Q_ONE ? 0x100000000ull : (u64)q32;
        if constexpr (ENT) {
            const float d = f32_from_orderable(key) - m;
            const float dd = q > 0ull ? d : 0.0f;                 // 0 where the mass is 0: the product below is finite
            h_sum += (u64)((double)q * (double)(-dd) * 65536.0);
        }
        return q32;
    };
    auto masses = [&](int i) {
        u32 k[4];
        if constexpr (NCH > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) k[e] = kreg[NCH ? i : 0][e];
        } else {
            u32 f = 0u;
            load_chunk<BF16>(a, row, tid + NT * i, k, f);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const u32 q32 = code(k[e]);
            if (NCH && !ENT) kreg[NCH ? i : 0][e] = q32;          // the mass takes the key's register; the ENT instances keep the key
            if (e & 1) __builtin_amdgcn_sched_barrier(0);         // two codes' polynomials in flight: the keys hold 64 registers already
        }
    };
    if constexpr (NCH > 0) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) masses(i);
    } else if (a.C >= 4) {
        for (int i = 0; i < n_it; ++i) masses(i);
    }
    if (tid == 0) {
#pragma unroll
        for (int e = 0; e < 3; ++e) code(sh.ktail[e]);            // a key 0 adds nothing
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        q_sum += shfl_xor_u64(q_sum, o);
        if constexpr (ENT) h_sum += shfl_xor_u64(h_sum, o);
    }
    if (lane == 0) {
        atomicAdd(&sh.qtot, q_sum);
        if constexpr (ENT) atomicAdd(&sh.hsum, h_sum);
    }
    __syncthreads();                                              // Q (and S) complete: from here on a thread reads only what it writes itself

    const u64 q_total = sh.qtot;
    const double inv_q = 1.0 / (double)q_total;
    if (tid == 0) {                                               // the row's transcendentals
        const double log_q = log((double)q_total * 2.3283064365386963e-10);        // Q * 2^-32 >= 1
        a.lse[r] = (float)((double)m + log_q);
        const double ent_e = ENT ? (double)sh.hsum / (65536.0 * (double)q_total) : 0.0;
        if (scored) {
            const float lp = (float)(((double)f32_from_orderable(tkey) - (double)m) - log_q);
            const float ratio = (float)exp((double)lp - (double)old_lp);
            const float lo = 1.0f - a.clip_lo, hi = 1.0f + a.clip_hi;
            const bool c_hi = adv > 0.0f && ratio > hi, c_lo = adv < 0.0f && ratio < lo;
            double e = 0.0;
            float kl = 0.0f;
            if (a.ref_lp) {
                const double u = (double)ref_lp - (double)lp;
                e = expm1(u);
                kl = (float)(e - u);
            }
            const double policy = (c_hi || c_lo || adv == 0.0f) ? 0.0 : (double)adv * (double)ratio;
            const double kl_term = (double)a.kl_coef * e;
            const double w = policy + kl_term;
            const float g = a.row_scale ? a.row_scale[r] : 1.0f;
            const float k = g * (float)w;
            a.logprob[r] = lp; a.ratio[r] = ratio; a.kl[r] = kl; a.coef[r] = k;
            a.flags[r] = (unsigned char)((c_hi ? 1 : 0) | (c_lo ? 2 : 0));
            if (a.entropy) a.entropy[r] = (float)(log_q + ent_e);
            sh.k = k; sh.kH = g * a.ent_coef; sh.E = ent_e;
        } else {
            a.logprob[r] = 0.0f; a.ratio[r] = 0.0f; a.kl[r] = 0.0f; a.coef[r] = 0.0f;
            a.flags[r] = 0;
            if (a.entropy) a.entropy[r] = 0.0f;
            atomicAdd(a.ignored, 1u);
        }
    }
    if (!want_grad) return;                                       // metrics only: nothing of a gradient is written
    if (!scored) {                                                // an ignored row: zeros, written after every read of the row
        zero_columns<BF16>(a, grow, 0L, a.V, tid);
        return;
    }
    __syncthreads();                                              // k, kH, E
    const float kv = sh.k, kH = sh.kH;
    const double ent_e = sh.E;
    const bool with_ent = a.ent_coef != 0.0f;                     // block-uniform

    // ---- sweep 3: p = q / Q, k p - k [i == t] (+ kH p (d + E)), the store ----
    auto grad_of = [&](u32 kq, u32 idx) {                         // kq: the key in the ENT instances and wherever the row is read again, else the mass
        if constexpr (ENT) {
            const u64 q = mass_of(kq, m);
            const double pd = (double)q * inv_q;
            const float x = kv * (float)pd - (idx == tidx ? kv : 0.0f);
            if (!with_ent) return x;
            const float d = f32_from_orderable(kq) - m;
            const float t = q > 0ull ? (float)(pd * ((double)d + ent_e)) : 0.0f;
            const float ht = kH * t;
            return x + ht;
        } else {
            const float p = (float)(mass_f64(kq) * inv_q);
            const float kp = kv * p;
            return kp - (idx == tidx ? kv : 0.0f);
        }
    };
    auto write = [&](int i) {
        const u32 i0 = 4u * (u32)(tid + NT * i);
        u32 q[4];
        if constexpr (NCH > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = kreg[NCH ? i : 0][e];
        } else {
            u32 f = 0u;
            load_chunk<BF16>(a, row, tid + NT * i, q, f);
            if constexpr (!ENT) {
#pragma unroll
                for (int e = 0; e < 4; ++e) q[e] = mass32(mass_of(q[e], m));
            }
        }
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = grad_of(q[e], i0 + e);
            if (ENT && (e & 1)) __builtin_amdgcn_sched_barrier(0); // two codes' polynomials and fp64 products in flight
        }
        if (i0 + 3u < (u32)a.C) store_four<BF16>(a, grow + (size_t)a.offset + i0, o);
        __builtin_amdgcn_sched_barrier(0);                        // one chunk's quotients in flight
    };
    if constexpr (NCH > 0) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) write(i);
    } else if (a.C >= 4) {
        for (int i = 0; i < n_it; ++i) write(i);
    }
    if (tid == 0) {
#pragma unroll
        for (int e = 0; e < 3; ++e)
            if (tail0 + e < (u32)a.C) {
                const u32 key = sh.ktail[e];
                store_one<BF16>(a, grow + (size_t)a.offset + tail0 + e, grad_of(ENT ? key : mass32(mass_of(key, m)), tail0 + e));
            }
    }
    zero_columns<BF16>(a, grow, 0L, a.offset, tid);
    zero_columns<BF16>(a, grow, a.offset + (long)a.C, a.V, tid);
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

int selftok_policy_rows(const void* logits, int dtype, int R, int C, long row_stride, long offset, const void* ids, int id_bytes, int rows_per_seq,
                        long id_seq_stride, long id_step_stride, long V, const float* row_scale, const float* old_logprob, const float* advantage,
                        const float* ref_logprob, float clip_lo, float clip_hi, float kl_coef, float ent_coef, float* logprob, float* lse, float* ratio, float* kl,
                        float* entropy, float* coef, unsigned char* flags, void* grad, long grad_stride, unsigned* bad, unsigned* ignored, hipStream_t stream)
{
    char msg[320];
    if (dtype != 0 && dtype != 1) {
        snprintf(msg, sizeof msg, "token_policy: dtype must be 0 (fp32) or 1 (bf16), got %d", dtype); set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (id_bytes != 4 && id_bytes != 8) {
        snprintf(msg, sizeof msg, "token_policy: id_bytes must be 4 (int32) or 8 (int64), got %d", id_bytes); set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (C < 1 || C > MAX_C) { snprintf(msg, sizeof msg, "token_policy: need 1 <= C <= %d, got %d", MAX_C, C); set_last_error(msg); return SELFTOK_EINVAL; }
    if (R < 0 || offset < 0 || row_stride < 0 || offset > row_stride || (long)C > row_stride - offset) {
        snprintf(msg, sizeof msg, "token_policy: need R >= 0 and the window [offset, offset + C) inside the row: R %d, offset %ld, C %d, row_stride %ld", R, offset, C,
                 row_stride);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (grad && (V < offset + (long)C || V > row_stride || (R > 1 && V > grad_stride))) {
        snprintf(msg, sizeof msg, "token_policy: need offset + C <= V <= row_stride and V <= grad_stride: V %ld, offset %ld, C %d, row_stride %ld, grad_stride %ld", V,
                 offset, C, row_stride, grad_stride);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (rows_per_seq < 1) {
        snprintf(msg, sizeof msg, "token_policy: need rows_per_seq >= 1, got %d", rows_per_seq); set_last_error(msg); return SELFTOK_EINVAL;
    }
    const float big = 3.4028234e38f;
    if (!(clip_lo >= 0.0f && clip_lo < 1.0f) || !(clip_hi >= 0.0f && clip_hi <= big)) {
        set_last_error("token_policy: need a clip range with 0 <= clip_lo < 1 and a finite clip_hi >= 0"); return SELFTOK_EINVAL;
    }
    if (!(kl_coef >= 0.0f && kl_coef <= big) || !(ent_coef >= 0.0f && ent_coef <= big)) {
        set_last_error("token_policy: need a finite kl_coef >= 0 and a finite ent_coef >= 0"); return SELFTOK_EINVAL;
    }
    if (kl_coef != 0.0f && !ref_logprob) { set_last_error("token_policy: kl_coef != 0 needs ref_logprob"); return SELFTOK_EINVAL; }
    if (R == 0) return SELFTOK_OK;
    if (!logits || !ids || !old_logprob || !advantage || !logprob || !lse || !ratio || !kl || !coef || !flags || !bad || !ignored) {
        set_last_error("token_policy: null pointer"); return SELFTOK_EINVAL;
    }
    const uintptr_t row_align = dtype == 1 ? 8 : 16;              // four codes: one vector load, one vector store
    if (((uintptr_t)logits % row_align) != 0 || ((uintptr_t)grad % row_align) != 0 || (offset & 3) != 0 ||
        (R > 1 && ((row_stride & 3) != 0 || (grad && (grad_stride & 3) != 0)))) {
        set_last_error("token_policy: misaligned rows: the logits and grad pointers must be aligned to four codes (16 bytes fp32, 8 bytes bf16), offset, row_stride "
                       "and grad_stride multiples of 4");
        return SELFTOK_EINVAL;
    }
    if (((uintptr_t)ids % (uintptr_t)id_bytes) != 0 || (((uintptr_t)row_scale | (uintptr_t)old_logprob | (uintptr_t)advantage | (uintptr_t)ref_logprob | (uintptr_t)logprob |
                                                          (uintptr_t)lse | (uintptr_t)ratio | (uintptr_t)kl | (uintptr_t)entropy | (uintptr_t)coef | (uintptr_t)bad |
                                                          (uintptr_t)ignored) & 3) != 0) {
        set_last_error("token_policy: row_scale, old_logprob, advantage, ref_logprob, the fp32 outputs, bad and ignored must be 4-byte aligned, ids aligned to id_bytes");
        return SELFTOK_EINVAL;
    }
    if (grad == logits) {
        if (grad_stride != row_stride) {
            set_last_error("token_policy: grad and logits overlap: in place needs grad == logits AND grad_stride == row_stride"); return SELFTOK_EINVAL;
        }
    } else if (grad) {                                            // the two extents, first element to last, must be disjoint
        const uintptr_t es = dtype == 1 ? 2 : 4;
        const uintptr_t l0 = (uintptr_t)logits, l1 = l0 + es * ((uintptr_t)(R - 1) * (uintptr_t)row_stride + (uintptr_t)offset + (uintptr_t)C);
        const uintptr_t g0 = (uintptr_t)grad, g1 = g0 + es * ((uintptr_t)(R - 1) * (uintptr_t)(R > 1 ? grad_stride : 0) + (uintptr_t)V);
        if (l0 < g1 && g0 < l1) {
            set_last_error("token_policy: grad and logits overlap: in place needs grad == logits AND grad_stride == row_stride"); return SELFTOK_EINVAL;
        }
    }
    PolicyArgs a;
    a.logits = logits; a.ids = ids; a.row_scale = row_scale; a.old_lp = old_logprob; a.adv = advantage; a.ref_lp = ref_logprob; a.grad = grad;
    a.logprob = logprob; a.lse = lse; a.ratio = ratio; a.kl = kl; a.entropy = entropy; a.coef = coef; a.flags = flags; a.bad = bad; a.ignored = ignored;
    a.row_stride = row_stride; a.offset = offset; a.id_seq_stride = id_seq_stride; a.id_step_stride = id_step_stride;
    a.grad_stride = (grad && R > 1) ? grad_stride : 0; a.V = grad ? V : 0;
    a.R = R; a.C = C; a.id_bytes = id_bytes; a.S = rows_per_seq;
    a.clip_lo = clip_lo; a.clip_hi = clip_hi; a.kl_coef = kl_coef; a.ent_coef = ent_coef;
    const unsigned gx = R < GRID_X ? (unsigned)R : (unsigned)GRID_X;
    const dim3 grid(gx, (unsigned)(((long)R + GRID_X - 1) / GRID_X)), block(NT);
    const bool bf = dtype == 1, ent = ent_coef != 0.0f || entropy != nullptr;
#define POLICY_LAUNCH(NCH, ENT)                                                                                               \
    do {                                                                                                                      \
        if (bf) hipLaunchKernelGGL((tok_policy_kernel<NCH, true, ENT>), grid, block, 0, stream, a);                           \
        else hipLaunchKernelGGL((tok_policy_kernel<NCH, false, ENT>), grid, block, 0, stream, a);                             \
    } while (0)
    // the register-resident instances, from the compiler's resource report: 16 chunks without the entropy sum (92 VGPRs), 8 with it (117); 10 and more chunks
    // with it spill, so those rows are streamed
    if (ent) {
        if (C <= SMALL_CH * 4 * NT) POLICY_LAUNCH(SMALL_CH, true);
        else if (C <= ENT_CH * 4 * NT) POLICY_LAUNCH(ENT_CH, true);
        else POLICY_LAUNCH(0, true);
    } else {
        if (C <= SMALL_CH * 4 * NT) POLICY_LAUNCH(SMALL_CH, false);
        else if (C <= REG_CH * 4 * NT) POLICY_LAUNCH(REG_CH, false);
        else POLICY_LAUNCH(0, false);
    }
#undef POLICY_LAUNCH
    return check_launch("token_policy kernel");
}

}  // extern "C"
