// Token distillation: one row of STUDENT logits and one row of TEACHER logits (optionally the guided teacher lu + s (lc - lu)) over the same window of C
// codes -> KL(teacher || student), the soft-target cross-entropy, the teacher's entropy, the student's log-sum-exp and the whole gradient row
// g (softmax_student - softmax_teacher), written over V columns and, if the caller says so, over the student logits themselves (include/selftok_hip_ext.h
// states the arithmetic of record: steps 1, 3 and 4 of the sampler's on either side, the scorer's entropy, and this entry's own cross term;
// selftoktokenizer_amd/losses.py and sampling.py are the host side; tests/token_distill_cases.py restates every step in numpy).
//
// The loss's shape (csrc/token_xent.hip): a workgroup of 512 threads owns a row, the grid is one workgroup per row (x = min(R, 65536), y the rest).  Thread
// t owns the 4-code chunks t, t + 512, .. of BOTH rows: one 16-byte load per chunk and input for fp32, 8 bytes for bf16, one vector store; the up to three
// codes of the partial chunk at the window's end are thread 0's, code by code.  Three sweeps: (1) the keys of both rows, the two maxima, NaN / +inf;
// (2) per code the two integer masses, the teacher's entropy term h and the cross term c = trunc(qA x 2^16) split into two 32-bit limbs, and the five integer
// sums QA, QB, S_A, S_lo, S_hi; (3) pB - pA, times g, the store.  Sweep (3) and every store are skipped when grad is null (metrics only).
// TWO rows' keys are live between the sweeps, so the register-resident instances hold a quarter of the loss's window:
//     tok_distill_kernel<2, ...>  C <= 4096    16 key registers    78 - 80 VGPRs    6 waves / SIMD
//     tok_distill_kernel<4, ...>  C <= 8192    32 key registers    110 - 113 VGPRs  4 waves / SIMD (two 512-thread workgroups per compute unit)
//     tok_distill_kernel<0, ...>  above        streamed            49 - 62 VGPRs    8 waves / SIMD
// (the compiler's resource report for gfx950 at this revision, no scratch anywhere.  Sweep (2) alone holds about 64 registers -- two mass polynomials, three
// fp64 products, five 64-bit sums -- so 6 chunks spilled 60 - 160 bytes per lane and 8 chunks 188 - 412 under the 128 registers of four waves per SIMD.)  At
// C <= 8192 both rows are read from memory ONCE: sweep (2) puts the mass of a code where its key was (Q_ONE = 0xFFFFFFFF stands for 2^32, as in the loss).
// Above that, sweeps (2) and (3) read the chunks again through the L2, as tok_xent_kernel<0, .> does.
// In place (grad == student): every thread's reads of the student row in sweeps (1) and (2) lie before the barrier that completes the five sums, and nothing
// is stored before that barrier.  After it the register-resident instances read no logit at all; the streamed instance re-reads only chunks the SAME thread
// stores, each before its own store, and a chunk past the window re-reads chunk 0 -- possibly overwritten by then -- and masks what it read to nothing; the
// partial chunk's keys wait in LDS.  The teacher rows may not overlap grad at all (refused on the host).  A bad row's and an ignored row's zeros are written
// after every read of the row (an ignored row reads none).  Every reduction is a maximum, an OR or an integer sum: any order gives the same bits.  No inline
// assembly, no scratch, no workspace, no state.
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
constexpr int REG_CH = 4;                                         // chunks of 4 codes of EITHER row a thread keeps in registers: 4 * 4 * 512 = 8192
constexpr int SMALL_CH = 2;                                       // 2 * 4 * 512 = 4096
constexpr int MAX_C = 65536;
constexpr int GRID_X = 65536;                                     // rows per grid row
constexpr u32 KEY_NEG_INF = 0x007FFFFFu;                          // f32_orderable(-inf)
constexpr u32 Q_ONE = 0xFFFFFFFFu;                                // the 32-bit image of the mass 2^32
constexpr u32 FLAG_BAD = 1u, FLAG_OVERFLOW = 2u;

struct DistArgs {
    const void* student; const void* teacher; const void* uncond; const float* row_scale; const unsigned char* row_mask; void* grad;
    float* kl; float* ce; float* h_teacher; float* lse; u32* bad; u32* ignored;
    long row_stride, t_stride, offset, grad_stride, V;
    int R, C;
    float cfg_scale;
};

struct Shared {
    u64 qa, qb, sa, slo, shi;
    u32 maxa, maxb, flags;
    u32 ta[3], tb[3];                                             // the keys of the partial chunk's up to three codes, teacher and student (0: no such code)
};

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int o)
{
    const u32 lo = __shfl_xor((u32)v, o, WAVE), hi = __shfl_xor((u32)(v >> 32), o, WAVE);
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ float widen(u16 h) { return __uint_as_float((u32)h << 16); }

// fp32 -> bf16, to nearest even, once; a NaN stays one
__device__ __forceinline__ u16 narrow(float f)
{
    const u32 u = __float_as_uint(f);
    const u32 r = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    return (u & 0x7FFFFFFFu) > 0x7F800000u ? (u16)0x7FC0u : (u16)r;
}

// the monotone uint32 key of a logit (-0.0 as +0.0); a NaN or +inf sets badf (the sampler's step 3)
__device__ __forceinline__ u32 key_of(float l, u32& badf)
{
    u32 u = __float_as_uint(l);
    if ((u & 0x7FFFFFFFu) == 0u) u = 0u;
    badf |= ((u & 0x7FFFFFFFu) > 0x7F800000u || u == 0x7F800000u) ? 1u : 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the teacher's logit and its key: the sampler's step 1 -- difference, product, sum, three roundings, none fused -- when guided; a NaN or +inf in either
// input or in the guided value sets badf
template <bool GUIDED>
__device__ __forceinline__ u32 teacher_key(float lc, float lu, float s, u32& badf)
{
    float l = lc;
    if (GUIDED) {
        key_of(lc, badf);
        key_of(lu, badf);
        const float diff = lc - lu;
        const float prod = s * diff;
        l = lu + prod;
    }
    return key_of(l, badf);
}

// the integer mass of a code d = l - m below the row maximum (the sampler's step 4, the same constants): exactly 2^32 at d = 0, 0 below -24, for -inf and
// for the NaN that a code past the window decodes to.  Branch-free, as the scorer's, and dd is handed back for the entropy term: q * (-dd) is 0 wherever q is.
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

__device__ __forceinline__ u32 mass32(u64 q) { return q > (u64)Q_ONE ? Q_ONE : (u32)q; }

__device__ __forceinline__ u32 mass32_of_key(u32 key, float m)
{
    float dd;
    return mass32(mass_of(f32_from_orderable(key) - m, dd));
}

__device__ __forceinline__ double mass_f64(u32 q32) { return q32 == Q_ONE ? 4294967296.0 : (double)q32; }

template <bool BF16>
__device__ __forceinline__ float elem_at(const void* base, size_t at)
{
    return BF16 ? widen(((const u16*)base)[at]) : ((const float*)base)[at];
}

template <bool BF16>
__device__ __forceinline__ void load_four(const void* base, size_t at, float l[4])
{
    if (BF16) {
        const u16x4 v = *(const u16x4*)((const u16*)base + at);
#pragma unroll
        for (int e = 0; e < 4; ++e) l[e] = widen(v[e]);
    } else {
        const f32x4 v = *(const f32x4*)((const float*)base + at);
#pragma unroll
        for (int e = 0; e < 4; ++e) l[e] = v[e];
    }
}

template <bool BF16>
__device__ __forceinline__ void store_one(const DistArgs& a, size_t at, float v)
{
    if (BF16) ((u16*)a.grad)[at] = narrow(v);
    else ((float*)a.grad)[at] = v;
}

template <bool BF16>
__device__ __forceinline__ void store_four(const DistArgs& a, size_t at, const float v[4])
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
__device__ __forceinline__ void zero_columns(const DistArgs& a, size_t base, long lo, long hi, int tid)
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

// the keys of the whole chunk j (codes 4 j .. 4 j + 3 < C) of both rows: one vector load per input; a chunk at or past the window's last, partial chunk reads
// chunk 0 instead (the caller has checked C >= 4) and gets keys 0 -- below every real key, a key 0 decodes to a NaN whose mass is 0 and whose cross term is
// masked -- so that the chunks of a thread are one basic block (the scorer's finding: with a branch per chunk the compiler issued every load first and spilled).
template <bool SBF, bool TBF, bool GUIDED>
__device__ __forceinline__ void load_chunk(const DistArgs& a, size_t srow, size_t trow, int j, u32 ka[4], u32 kb[4], u32& badf)
{
    const u32 i0 = 4u * (u32)j;
    const u32 in = (u32)((int)(i0 + 3u - (u32)a.C) >> 31);        // all ones inside the window; a vector mask
    const u32 i = i0 & in;
    float lc[4], lu[4] = {0.0f, 0.0f, 0.0f, 0.0f}, b[4];
    load_four<TBF>(a.teacher, trow + i, lc);
    if (GUIDED) load_four<TBF>(a.uncond, trow + i, lu);
    load_four<SBF>(a.student, srow + i, b);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        u32 f = 0u;
        const u32 key_a = teacher_key<GUIDED>(lc[e], lu[e], a.cfg_scale, f);
        const u32 key_b = key_of(b[e], f);
        ka[e] = key_a & in;
        kb[e] = key_b & in;
        badf |= f & in;
    }
}

template <int NCH, bool SBF, bool TBF, bool GUIDED>
__global__ void __launch_bounds__(NT, 4) tok_distill_kernel(const DistArgs a)
{
    __shared__ Shared sh;
    const long r = (long)blockIdx.y * GRID_X + (long)blockIdx.x;
    if (r >= (long)a.R) return;                                   // the last grid row: block-uniform
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t srow = (size_t)r * (size_t)a.row_stride + (size_t)a.offset;
    const size_t trow = (size_t)r * (size_t)a.t_stride + (size_t)a.offset;
    const size_t grow = (size_t)r * (size_t)a.grad_stride;        // the gradient row's column 0
    const bool with_grad = a.grad != nullptr;                     // block-uniform
    const int n_it = NCH ? NCH : (a.C + 4 * NT - 1) / (4 * NT);
    const u32 tail0 = (u32)a.C & ~3u;                             // the first code of the partial chunk

    // an ignored row: no logit of it is read (every thread reads the same mask byte)
    if (a.row_mask && __builtin_amdgcn_readfirstlane((int)a.row_mask[r]) == 0) {
        if (with_grad) zero_columns<SBF>(a, grow, 0L, a.V, tid);
        if (tid == 0) {
            a.kl[r] = 0.0f; a.ce[r] = 0.0f; a.h_teacher[r] = 0.0f; a.lse[r] = 0.0f;
            atomicAdd(a.ignored, 1u);
        }
        return;
    }

    if (tid == 0) {
        sh.qa = 0ull; sh.qb = 0ull; sh.sa = 0ull; sh.slo = 0ull; sh.shi = 0ull; sh.maxa = 0u; sh.maxb = 0u; sh.flags = 0u;
#pragma unroll
        for (int e = 0; e < 3; ++e) { sh.ta[e] = 0u; sh.tb[e] = 0u; }
    }
    __syncthreads();

    // ---- sweep 1, the one read of both rows at C <= 8192: keys, the two maxima, NaN / +inf ----
    u32 kra[NCH ? NCH : 1][4], krb[NCH ? NCH : 1][4];
    u32 mxa = 0u, mxb = 0u, badf = 0u;
    auto first_read = [&](int i) {
        u32 ka[4], kb[4];
        load_chunk<SBF, TBF, GUIDED>(a, srow, trow, tid + NT * i, ka, kb, badf);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (NCH) { kra[NCH ? i : 0][e] = ka[e]; krb[NCH ? i : 0][e] = kb[e]; }
            mxa = ka[e] > mxa ? ka[e] : mxa;
            mxb = kb[e] > mxb ? kb[e] : mxb;
        }
        if ((i & 1) == 1) __builtin_amdgcn_sched_barrier(0);      // two chunks' loads in flight per thread (four to six vector loads), not all of them
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
            for (int e = 0; e < 4; ++e) { kra[i][e] = 0u; krb[i][e] = 0u; }
    }
    if (tid == 0) {
#pragma unroll
        for (int e = 0; e < 3; ++e)
            if (tail0 + e < (u32)a.C) {
                const float lc = elem_at<TBF>(a.teacher, trow + tail0 + e);
                const float lu = GUIDED ? elem_at<TBF>(a.uncond, trow + tail0 + e) : 0.0f;
                const u32 key_a = teacher_key<GUIDED>(lc, lu, a.cfg_scale, badf);
                const u32 key_b = key_of(elem_at<SBF>(a.student, srow + tail0 + e), badf);
                sh.ta[e] = key_a; sh.tb[e] = key_b;
                mxa = key_a > mxa ? key_a : mxa;
                mxb = key_b > mxb ? key_b : mxb;
            }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u32 va = __shfl_xor(mxa, o, WAVE), vb = __shfl_xor(mxb, o, WAVE);
        mxa = va > mxa ? va : mxa;
        mxb = vb > mxb ? vb : mxb;
    }
    if (lane == 0) { atomicMax(&sh.maxa, mxa); atomicMax(&sh.maxb, mxb); }
    if (__ballot(badf != 0u) != 0ull && lane == 0) atomicOr(&sh.flags, FLAG_BAD);
    __syncthreads();

    const u32 maxa = (u32)__builtin_amdgcn_readfirstlane((int)sh.maxa), maxb = (u32)__builtin_amdgcn_readfirstlane((int)sh.maxb);
    if ((sh.flags & FLAG_BAD) != 0u || maxa <= KEY_NEG_INF || maxb <= KEY_NEG_INF) {   // a bad row, block-uniform: every read of it lies before the barrier above
        if (with_grad) zero_columns<SBF>(a, grow, 0L, a.V, tid);
        if (tid == 0) {
            const float nan = __uint_as_float(0x7FC00000u);
            a.kl[r] = nan; a.ce[r] = nan; a.h_teacher[r] = nan; a.lse[r] = nan;
            atomicAdd(a.bad, 1u);
        }
        return;
    }
    const float ma = f32_from_orderable(maxa), mb = f32_from_orderable(maxb);
    const double mbd = (double)mb;

    // ---- sweep 2: the two masses, the teacher's entropy term, the cross term, the five integer sums ----
    u64 qa_sum = 0ull, qb_sum = 0ull, sa_sum = 0ull, lo_sum = 0ull, hi_sum = 0ull;
    u32 ovf = 0u;
    auto code = [&](u32 key_a, u32 key_b, u32& qa32, u32& qb32) {
        float dda, ddb;
        const u64 qa = mass_of(f32_from_orderable(key_a) - ma, dda);
        const float b = f32_from_orderable(key_b);
        const u64 qb = mass_of(b - mb, ddb);
        qa_sum += qa;
        qb_sum += qb;
        const double qad = (double)qa;
        sa_sum += (u64)(qad * (double)(-dda) * 65536.0);                     // 0 where qa is 0: dda is finite
        const double x = mbd - (double)b;                                    // >= 0, +inf for a student at -inf, NaN past the window
        const bool live = qa != 0ull, fits = x < 32768.0;
        ovf |= (live && !fits) ? 1u : 0u;
        const double xs = (live && fits) ? x : 0.0;
        const u64 c = (u64)((qad * xs) * 65536.0);                           // below 2^63
        lo_sum += c & 0xFFFFFFFFull;
        hi_sum += c >> 32;
        qa32 = mass32(qa);
        qb32 = mass32(qb);
    };
    auto masses = [&](int i) {
        u32 ka[4], kb[4];
        if constexpr (NCH > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { ka[e] = kra[NCH ? i : 0][e]; kb[e] = krb[NCH ? i : 0][e]; }
        } else {
            u32 f = 0u;
            load_chunk<SBF, TBF, GUIDED>(a, srow, trow, tid + NT * i, ka, kb, f);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            u32 qa32, qb32;
            code(ka[e], kb[e], qa32, qb32);
            if (NCH) { kra[NCH ? i : 0][e] = qa32; krb[NCH ? i : 0][e] = qb32; }      // the masses take the keys' registers
            __builtin_amdgcn_sched_barrier(0);                    // one code's two polynomials and fp64 terms in flight
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
        for (int e = 0; e < 3; ++e) { u32 qa32, qb32; code(sh.ta[e], sh.tb[e], qa32, qb32); }      // keys 0 (no such code) add nothing
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        qa_sum += shfl_xor_u64(qa_sum, o);
        qb_sum += shfl_xor_u64(qb_sum, o);
        sa_sum += shfl_xor_u64(sa_sum, o);
        lo_sum += shfl_xor_u64(lo_sum, o);
        hi_sum += shfl_xor_u64(hi_sum, o);
    }
    if (lane == 0) { atomicAdd(&sh.qa, qa_sum); atomicAdd(&sh.qb, qb_sum); atomicAdd(&sh.sa, sa_sum); atomicAdd(&sh.slo, lo_sum); atomicAdd(&sh.shi, hi_sum); }
    if (__ballot(ovf != 0u) != 0ull && lane == 0) atomicOr(&sh.flags, FLAG_OVERFLOW);
    __syncthreads();                                              // the sums are complete and the student row is consumed: from here on a thread reads only what it writes itself

    const double qad = (double)sh.qa, qbd = (double)sh.qb;
    if (tid == 0) {
        const double la = log(qad * 2.3283064365386963e-10), lb = log(qbd * 2.3283064365386963e-10);      // Q * 2^-32 >= 1
        const double ea = (double)sh.sa / (65536.0 * qad);
        const double x = (double)sh.shi * 4294967296.0 + (double)sh.slo;
        const double ex = x / (65536.0 * qad);
        const bool over = (sh.flags & FLAG_OVERFLOW) != 0u;
        const float inf = __uint_as_float(0x7F800000u);
        a.lse[r] = (float)(mbd + lb);
        a.h_teacher[r] = (float)(la + ea);
        a.ce[r] = over ? inf : (float)(lb + ex);
        a.kl[r] = over ? inf : (float)(((lb - la) + ex) - ea);
    }
    if (!with_grad) return;

    // ---- sweep 3: pA = qA / QA, pB = qB / QB, g (pB - pA), the store ----
    const double inv_qa = 1.0 / qad, inv_qb = 1.0 / qbd;
    const float g = a.row_scale ? a.row_scale[r] : 1.0f;
    auto grad_of = [&](u32 qa32, u32 qb32) {
        const float pa = (float)(mass_f64(qa32) * inv_qa);
        const float pb = (float)(mass_f64(qb32) * inv_qb);
        const float diff = pb - pa;
        return g * diff;
    };
    auto write = [&](int i) {
        const u32 i0 = 4u * (u32)(tid + NT * i);
        u32 qa[4], qb[4];
        if constexpr (NCH > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { qa[e] = kra[NCH ? i : 0][e]; qb[e] = krb[NCH ? i : 0][e]; }
        } else {
            u32 ka[4], kb[4], f = 0u;
            load_chunk<SBF, TBF, GUIDED>(a, srow, trow, tid + NT * i, ka, kb, f);
#pragma unroll
            for (int e = 0; e < 4; ++e) { qa[e] = mass32_of_key(ka[e], ma); qb[e] = mass32_of_key(kb[e], mb); }
        }
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = grad_of(qa[e], qb[e]);
        if (i0 + 3u < (u32)a.C) store_four<SBF>(a, grow + (size_t)a.offset + i0, o);
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
            if (tail0 + e < (u32)a.C) store_one<SBF>(a, grow + (size_t)a.offset + tail0 + e, grad_of(mass32_of_key(sh.ta[e], ma), mass32_of_key(sh.tb[e], mb)));
    }
    zero_columns<SBF>(a, grow, 0L, a.offset, tid);
    zero_columns<SBF>(a, grow, a.offset + (long)a.C, a.V, tid);
}

// [p0, p1) and [q0, q1) intersect
inline bool extents_meet(uintptr_t p0, uintptr_t p1, uintptr_t q0, uintptr_t q1) { return p0 < q1 && q0 < p1; }

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

int selftok_distill_rows(const void* student, int dtype, const void* teacher, const void* teacher_uncond, int teacher_dtype, int R, int C, long row_stride,
                         long teacher_stride, long offset, float cfg_scale, long V, const float* row_scale, const unsigned char* row_mask, float* kl, float* ce,
                         float* h_teacher, float* lse_student, void* grad, long grad_stride, unsigned* bad, unsigned* ignored, hipStream_t stream)
{
    char msg[360];
    if ((dtype != 0 && dtype != 1) || (teacher_dtype != 0 && teacher_dtype != 1)) {
        snprintf(msg, sizeof msg, "token_distill: dtype and teacher_dtype must be 0 (fp32) or 1 (bf16), got %d and %d", dtype, teacher_dtype);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (C < 1 || C > MAX_C) { snprintf(msg, sizeof msg, "token_distill: need 1 <= C <= %d, got %d", MAX_C, C); set_last_error(msg); return SELFTOK_EINVAL; }
    if (R < 0 || offset < 0 || row_stride < 0 || teacher_stride < 0 || offset > row_stride || (long)C > row_stride - offset || offset > teacher_stride ||
        (long)C > teacher_stride - offset) {
        snprintf(msg, sizeof msg, "token_distill: need R >= 0 and the window [offset, offset + C) inside the student's and the teacher's row: R %d, offset %ld, C %d, "
                 "row_stride %ld, teacher_stride %ld", R, offset, C, row_stride, teacher_stride);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (grad && (V < offset + (long)C || V > row_stride || (R > 1 && V > grad_stride))) {
        snprintf(msg, sizeof msg, "token_distill: need offset + C <= V <= row_stride and V <= grad_stride: V %ld, offset %ld, C %d, row_stride %ld, grad_stride %ld", V,
                 offset, C, row_stride, grad_stride);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (teacher_uncond && !(fabsf(cfg_scale) <= 3.4028234e38f)) { set_last_error("token_distill: need a finite cfg_scale with teacher_uncond"); return SELFTOK_EINVAL; }
    if (R == 0) return SELFTOK_OK;
    if (!student || !teacher || !kl || !ce || !h_teacher || !lse_student || !bad || !ignored) { set_last_error("token_distill: null pointer"); return SELFTOK_EINVAL; }
    const uintptr_t s_align = dtype == 1 ? 8 : 16, t_align = teacher_dtype == 1 ? 8 : 16;          // four codes: one vector load, one vector store
    if (((uintptr_t)student % s_align) != 0 || ((uintptr_t)grad % s_align) != 0 || ((uintptr_t)teacher % t_align) != 0 || ((uintptr_t)teacher_uncond % t_align) != 0 ||
        (offset & 3) != 0 || (R > 1 && ((row_stride & 3) != 0 || (teacher_stride & 3) != 0 || (grad && (grad_stride & 3) != 0)))) {
        set_last_error("token_distill: misaligned rows: the student, teacher, teacher_uncond and grad pointers must be aligned to four codes (16 bytes fp32, 8 bytes "
                       "bf16), offset, row_stride, teacher_stride and grad_stride multiples of 4");
        return SELFTOK_EINVAL;
    }
    if (((uintptr_t)kl & 3) != 0 || ((uintptr_t)ce & 3) != 0 || ((uintptr_t)h_teacher & 3) != 0 || ((uintptr_t)lse_student & 3) != 0 || ((uintptr_t)row_scale & 3) != 0 ||
        ((uintptr_t)bad & 3) != 0 || ((uintptr_t)ignored & 3) != 0) {
        set_last_error("token_distill: kl, ce, h_teacher, lse_student, row_scale, bad and ignored must be 4-byte aligned");
        return SELFTOK_EINVAL;
    }
    if (grad) {                                                   // extents, first element to last
        const uintptr_t es = dtype == 1 ? 2 : 4, et = teacher_dtype == 1 ? 2 : 4;
        const uintptr_t rows = (uintptr_t)(R - 1);
        const uintptr_t s0 = (uintptr_t)student, s1 = s0 + es * (rows * (uintptr_t)row_stride + (uintptr_t)offset + (uintptr_t)C);
        const uintptr_t g0 = (uintptr_t)grad, g1 = g0 + es * (rows * (uintptr_t)(R > 1 ? grad_stride : 0) + (uintptr_t)V);
        const uintptr_t t_len = et * (rows * (uintptr_t)teacher_stride + (uintptr_t)offset + (uintptr_t)C);
        if (grad == student ? grad_stride != row_stride : extents_meet(s0, s1, g0, g1)) {
            set_last_error("token_distill: grad and student overlap: in place needs grad == student AND grad_stride == row_stride"); return SELFTOK_EINVAL;
        }
        if (extents_meet((uintptr_t)teacher, (uintptr_t)teacher + t_len, g0, g1) ||
            (teacher_uncond && extents_meet((uintptr_t)teacher_uncond, (uintptr_t)teacher_uncond + t_len, g0, g1))) {
            set_last_error("token_distill: grad and the teacher overlap: the teacher rows are read after the first store"); return SELFTOK_EINVAL;
        }
    }
    DistArgs a;
    a.student = student; a.teacher = teacher; a.uncond = teacher_uncond; a.row_scale = row_scale; a.row_mask = row_mask; a.grad = grad;
    a.kl = kl; a.ce = ce; a.h_teacher = h_teacher; a.lse = lse_student; a.bad = bad; a.ignored = ignored;
    a.row_stride = row_stride; a.t_stride = teacher_stride; a.offset = offset; a.grad_stride = R > 1 ? grad_stride : 0; a.V = V;
    a.R = R; a.C = C;
    a.cfg_scale = cfg_scale;
    const unsigned gx = R < GRID_X ? (unsigned)R : (unsigned)GRID_X;
    const dim3 grid(gx, (unsigned)(((long)R + GRID_X - 1) / GRID_X)), block(NT);
    const bool sb = dtype == 1, tb = teacher_dtype == 1, gd = teacher_uncond != nullptr;
#define DISTILL_LAUNCH3(NCH, SB, TB)                                                                                          \
    do {                                                                                                                      \
        if (gd) hipLaunchKernelGGL((tok_distill_kernel<NCH, SB, TB, true>), grid, block, 0, stream, a);                       \
        else hipLaunchKernelGGL((tok_distill_kernel<NCH, SB, TB, false>), grid, block, 0, stream, a);                         \
    } while (0)
#define DISTILL_LAUNCH(NCH)                                                                                                   \
    do {                                                                                                                      \
        if (sb && tb) DISTILL_LAUNCH3(NCH, true, true);                                                                       \
        else if (sb) DISTILL_LAUNCH3(NCH, true, false);                                                                       \
        else if (tb) DISTILL_LAUNCH3(NCH, false, true);                                                                       \
        else DISTILL_LAUNCH3(NCH, false, false);                                                                              \
    } while (0)
    if (C <= SMALL_CH * 4 * NT) DISTILL_LAUNCH(SMALL_CH);
    else if (C <= REG_CH * 4 * NT) DISTILL_LAUNCH(REG_CH);
    else DISTILL_LAUNCH(0);
#undef DISTILL_LAUNCH
#undef DISTILL_LAUNCH3
    return check_launch("token_distill kernel");
}

}  // extern "C"
