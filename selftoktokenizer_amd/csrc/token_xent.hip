// Token loss: one row of AR logits over a window of C codes and ONE KNOWN target id -> the row's negative log-likelihood, its log-sum-exp and the whole
// gradient row a * softmax - g * onehot, written over V columns and, if the caller says so, over the logits themselves (include/selftok_hip_ext.h states the
// arithmetic of record: steps 1 - 4 of the sampler's at temperature 1 without guidance, and the loss's own block; selftoktokenizer_amd/losses.py is the host
// side; tests/token_xent_cases.py restates every step in numpy).
//
// The scorer's shape (csrc/token_score.hip): a workgroup of 512 threads owns a row, the grid is one workgroup per row (x = min(R, 65536), y the rest).  Thread
// t owns the 4-code chunks t, t + 512, ..: one 16-byte load and one 16-byte store per chunk for fp32, 8 bytes for bf16; the up to three codes of the partial
// chunk at the window's end are thread 0's, code by code.  Three sweeps: (1) keys, the maximum, NaN / +inf; (2) the integer mass q of every code and their
// sum Q_total; (3) p = q / Q_total, the gradient, the store.  At C <= 32768 the row is read from memory ONCE (tok_xent_kernel<16, .>; <2, .> for C <= 4096):
// the keys stay in registers between (1) and (2), and (2) puts the mass of a code where its key was -- a mass is a multiple of 256 from 2^31 on, so
// 0xFFFFFFFF is free to stand for 2^32 and 32 bits hold it.  Above that (tok_xent_kernel<0, .>) sweeps (2) and (3) read the chunks again through the L2.
// In place (grad == logits): a thread stores only chunks it has itself loaded in its last sweep, and nothing is stored before the barrier that completes
// Q_total, after which no thread needs a value it has not loaded itself -- a chunk past the window re-reads chunk 0, possibly overwritten by then, and masks
// what it read to nothing.  Every reduction is a maximum or an integer sum: any order gives the same bits.  No inline assembly, no scratch, no state.
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
constexpr u32 Q_ONE = 0xFFFFFFFFu;                                // the 32-bit image of the mass 2^32

struct XentArgs {
    const void* logits; const void* ids; const float* row_scale; void* grad;
    float* nll; float* lse; u32* bad; u32* ignored;
    long row_stride, offset, id_seq_stride, id_step_stride, grad_stride, V;
    int R, C, id_bytes, S;
    float z_coef;
};

struct Shared {
    u64 qtot;
    u32 maxkey, flags;
    float a;
    u32 ktail[3];                                                 // the keys of the partial chunk's up to three codes (0: no such code)
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

// the integer mass of a code d = l - m below the row maximum (the sampler's step 4, the same constants): exactly 2^32 at d = 0, 0 below -24, for -inf and
// for the NaN that a code past the window decodes to.  Branch-free, as the scorer's: a chunk of a sweep stays one basic block.
__device__ __forceinline__ u64 mass_of(float d)
{
    const bool ok = d >= -24.0f;
    const float dd = ok ? d : 0.0f;
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

// the mass in 32 bits: it is a multiple of 256 from 2^31 on and at most 2^32, so Q_ONE = 0xFFFFFFFF is free to stand for 2^32.  (A float -> uint32 conversion
// in mass_of itself would save ten instructions per code; every form of it tried made the 16-chunk kernels spill -- 108 bytes of scratch -- so it is not done.)
__device__ __forceinline__ u32 mass32_of_key(u32 key, float m)
{
    const u64 q = mass_of(f32_from_orderable(key) - m);
    return q > (u64)Q_ONE ? Q_ONE : (u32)q;
}

__device__ __forceinline__ double mass_f64(u32 q32) { return q32 == Q_ONE ? 4294967296.0 : (double)q32; }

template <bool BF16>
__device__ __forceinline__ float logit_at(const XentArgs& a, size_t row, u32 idx)
{
    return BF16 ? widen(((const u16*)a.logits)[row + idx]) : ((const float*)a.logits)[row + idx];
}

template <bool BF16>
__device__ __forceinline__ void store_one(const XentArgs& a, size_t at, float v)
{
    if (BF16) ((u16*)a.grad)[at] = narrow(v);
    else ((float*)a.grad)[at] = v;
}

template <bool BF16>
__device__ __forceinline__ void store_four(const XentArgs& a, size_t at, const float v[4])
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
__device__ __forceinline__ void zero_columns(const XentArgs& a, size_t base, long lo, long hi, int tid)
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
// basic block (the scorer's finding: with a branch per chunk the compiler issued every load first and spilled).
template <bool BF16>
__device__ __forceinline__ void load_chunk(const XentArgs& a, size_t row, int j, u32 k[4], u32& badf)
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

template <int NCH, bool BF16>
__global__ void __launch_bounds__(NT, 4) tok_xent_kernel(const XentArgs a)
{
    __shared__ Shared sh;
    const long r = (long)blockIdx.y * GRID_X + (long)blockIdx.x;
    if (r >= (long)a.R) return;                                   // the last grid row: block-uniform
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t row = (size_t)r * (size_t)a.row_stride + (size_t)a.offset;
    const size_t grow = (size_t)r * (size_t)a.grad_stride;        // the gradient row's column 0
    const int n_it = NCH ? NCH : (a.C + 4 * NT - 1) / (4 * NT);
    const u32 tail0 = (u32)a.C & ~3u;                             // the first code of the partial chunk

    if (tid == 0) { sh.qtot = 0ull; sh.maxkey = 0u; sh.flags = 0u; sh.a = 0.0f; sh.ktail[0] = 0u; sh.ktail[1] = 0u; sh.ktail[2] = 0u; }

    // the target: every thread reads the same element
    const long io = (r / a.S) * a.id_seq_stride + (r % a.S) * a.id_step_stride;
    const long long tv_v = a.id_bytes == 8 ? ((const long long*)a.ids)[io] : (long long)((const int*)a.ids)[io];
    const long long tv = (long long)(((u64)(u32)__builtin_amdgcn_readfirstlane((int)((u64)tv_v >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)tv_v));
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

    const u32 maxkey = (u32)__builtin_amdgcn_readfirstlane((int)sh.maxkey);
    if (sh.flags != 0u || maxkey <= KEY_NEG_INF || tv >= (long long)a.C) {             // a bad row, block-uniform: every read of it lies before the barrier above
        zero_columns<BF16>(a, grow, 0L, a.V, tid);
        if (tid == 0) {
            a.nll[r] = __uint_as_float(0x7FC00000u);
            a.lse[r] = __uint_as_float(0x7FC00000u);
            atomicAdd(a.bad, 1u);
        }
        return;
    }
    const float m = f32_from_orderable(maxkey);
    const bool scored = tv >= 0;
    const u32 tidx = scored ? (u32)tv : 0xFFFFFFFFu;              // no code has this index
    u32 tkey = 0u;
    if (scored) { u32 f = 0u; tkey = (u32)__builtin_amdgcn_readfirstlane((int)key_of(logit_at<BF16>(a, row, tidx), f)); }

    // ---- sweep 2: the integer masses and their sum ----
    u64 q_sum = 0ull;
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
            const u32 q32 = mass32_of_key(k[e], m);
            q_sum += q32 == Q_ONE ? 0x100000000ull : (u64)q32;
            if (NCH) kreg[NCH ? i : 0][e] = q32;                  // the mass takes the key's register
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
        for (int e = 0; e < 3; ++e) { const u32 q32 = mass32_of_key(sh.ktail[e], m); q_sum += q32 == Q_ONE ? 0x100000000ull : (u64)q32; }   // a key 0 adds nothing
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q_sum += shfl_xor_u64(q_sum, o);
    if (lane == 0) atomicAdd(&sh.qtot, q_sum);
    __syncthreads();                                              // Q_total is complete: from here on a thread reads only what it writes itself

    const u64 q_total = sh.qtot;
    const double inv_q = 1.0 / (double)q_total;
    const float g = scored ? (a.row_scale ? a.row_scale[r] : 1.0f) : 0.0f;
    const bool with_z = a.z_coef != 0.0f;                         // block-uniform
    if (tid == 0) {
        const double log_z = log((double)q_total * 2.3283064365386963e-10);       // Q_total * 2^-32 >= 1
        const double lse = (double)m + log_z;
        a.lse[r] = (float)lse;
        if (scored) {
            a.nll[r] = (float)(-(((double)f32_from_orderable(tkey) - (double)m) - log_z));
            if (with_z) {
                const double twice = 2.0 * (double)a.z_coef;
                const double zl = twice * lse;
                sh.a = g * (float)(1.0 + zl);
            }
        } else {
            a.nll[r] = 0.0f;
            atomicAdd(a.ignored, 1u);
        }
    }
    float av = g;                                                 // z_coef == 0: the factor is exactly 1
    if (with_z) {
        __syncthreads();
        av = sh.a;                                                // 0 on an ignored row, as g is
    }

    // ---- sweep 3: p = q / Q_total, a p - g [i == t], the store ----
    auto grad_of = [&](u32 q32, u32 idx) {
        const float p = (float)(mass_f64(q32) * inv_q);
        const float ap = av * p;
        return ap - (idx == tidx ? g : 0.0f);
    };
    auto write = [&](int i) {
        const u32 i0 = 4u * (u32)(tid + NT * i);
        u32 q[4];
        if constexpr (NCH > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = kreg[NCH ? i : 0][e];
        } else {
            u32 k[4], f = 0u;
            load_chunk<BF16>(a, row, tid + NT * i, k, f);
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = mass32_of_key(k[e], m);
        }
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = grad_of(q[e], i0 + e);
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
            if (tail0 + e < (u32)a.C) store_one<BF16>(a, grow + (size_t)a.offset + tail0 + e, grad_of(mass32_of_key(sh.ktail[e], m), tail0 + e));
    }
    zero_columns<BF16>(a, grow, 0L, a.offset, tid);
    zero_columns<BF16>(a, grow, a.offset + (long)a.C, a.V, tid);
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

int selftok_xent_rows(const void* logits, int dtype, int R, int C, long row_stride, long offset, const void* ids, int id_bytes, int rows_per_seq,
                      long id_seq_stride, long id_step_stride, long V, const float* row_scale, float z_coef, float* nll, float* lse, void* grad,
                      long grad_stride, unsigned* bad, unsigned* ignored, hipStream_t stream)
{
    char msg[320];
    if (dtype != 0 && dtype != 1) {
        snprintf(msg, sizeof msg, "token_xent: dtype must be 0 (fp32) or 1 (bf16), got %d", dtype); set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (id_bytes != 4 && id_bytes != 8) {
        snprintf(msg, sizeof msg, "token_xent: id_bytes must be 4 (int32) or 8 (int64), got %d", id_bytes); set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (C < 1 || C > MAX_C) { snprintf(msg, sizeof msg, "token_xent: need 1 <= C <= %d, got %d", MAX_C, C); set_last_error(msg); return SELFTOK_EINVAL; }
    if (R < 0 || offset < 0 || row_stride < 0 || offset > row_stride || (long)C > row_stride - offset) {
        snprintf(msg, sizeof msg, "token_xent: need R >= 0 and the window [offset, offset + C) inside the row: R %d, offset %ld, C %d, row_stride %ld", R, offset, C,
                 row_stride);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (V < offset + (long)C || V > row_stride || (R > 1 && V > grad_stride)) {
        snprintf(msg, sizeof msg, "token_xent: need offset + C <= V <= row_stride and V <= grad_stride: V %ld, offset %ld, C %d, row_stride %ld, grad_stride %ld", V,
                 offset, C, row_stride, grad_stride);
        set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (rows_per_seq < 1) {
        snprintf(msg, sizeof msg, "token_xent: need rows_per_seq >= 1, got %d", rows_per_seq); set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (!(z_coef >= 0.0f) || isinf(z_coef)) { set_last_error("token_xent: need a finite z_coef >= 0"); return SELFTOK_EINVAL; }
    if (R == 0) return SELFTOK_OK;
    if (!logits || !ids || !nll || !lse || !grad || !bad || !ignored) { set_last_error("token_xent: null pointer"); return SELFTOK_EINVAL; }
    const uintptr_t row_align = dtype == 1 ? 8 : 16;              // four codes: one vector load, one vector store
    if (((uintptr_t)logits % row_align) != 0 || ((uintptr_t)grad % row_align) != 0 || (offset & 3) != 0 || (R > 1 && ((row_stride & 3) != 0 || (grad_stride & 3) != 0))) {
        set_last_error("token_xent: misaligned rows: the logits and grad pointers must be aligned to four codes (16 bytes fp32, 8 bytes bf16), offset, row_stride "
                       "and grad_stride multiples of 4");
        return SELFTOK_EINVAL;
    }
    if (((uintptr_t)ids % (uintptr_t)id_bytes) != 0 || ((uintptr_t)nll & 3) != 0 || ((uintptr_t)lse & 3) != 0 || ((uintptr_t)row_scale & 3) != 0 ||
        ((uintptr_t)bad & 3) != 0 || ((uintptr_t)ignored & 3) != 0) {
        set_last_error("token_xent: nll, lse, row_scale, bad and ignored must be 4-byte aligned, ids aligned to id_bytes");
        return SELFTOK_EINVAL;
    }
    if (grad == logits) {
        if (grad_stride != row_stride) {
            set_last_error("token_xent: grad and logits overlap: in place needs grad == logits AND grad_stride == row_stride"); return SELFTOK_EINVAL;
        }
    } else {                                                      // the two extents, first element to last, must be disjoint
        const uintptr_t es = dtype == 1 ? 2 : 4;
        const uintptr_t l0 = (uintptr_t)logits, l1 = l0 + es * ((uintptr_t)(R - 1) * (uintptr_t)row_stride + (uintptr_t)offset + (uintptr_t)C);
        const uintptr_t g0 = (uintptr_t)grad, g1 = g0 + es * ((uintptr_t)(R - 1) * (uintptr_t)(R > 1 ? grad_stride : 0) + (uintptr_t)V);
        if (l0 < g1 && g0 < l1) {
            set_last_error("token_xent: grad and logits overlap: in place needs grad == logits AND grad_stride == row_stride"); return SELFTOK_EINVAL;
        }
    }
    XentArgs a;
    a.logits = logits; a.ids = ids; a.row_scale = row_scale; a.grad = grad;
    a.nll = nll; a.lse = lse; a.bad = bad; a.ignored = ignored;
    a.row_stride = row_stride; a.offset = offset; a.id_seq_stride = id_seq_stride; a.id_step_stride = id_step_stride;
    a.grad_stride = R > 1 ? grad_stride : 0; a.V = V;
    a.R = R; a.C = C; a.id_bytes = id_bytes; a.S = rows_per_seq;
    a.z_coef = z_coef;
    const unsigned gx = R < GRID_X ? (unsigned)R : (unsigned)GRID_X;
    const dim3 grid(gx, (unsigned)(((long)R + GRID_X - 1) / GRID_X)), block(NT);
    const bool bf = dtype == 1;
#define XENT_LAUNCH(NCH)                                                                                                      \
    do {                                                                                                                      \
        if (bf) hipLaunchKernelGGL((tok_xent_kernel<NCH, true>), grid, block, 0, stream, a);                                  \
        else hipLaunchKernelGGL((tok_xent_kernel<NCH, false>), grid, block, 0, stream, a);                                    \
    } while (0)
    if (C <= SMALL_CH * 4 * NT) XENT_LAUNCH(SMALL_CH);
    else if (C <= REG_CH * 4 * NT) XENT_LAUNCH(REG_CH);
    else XENT_LAUNCH(0);
#undef XENT_LAUNCH
    return check_launch("token_xent kernel");
}

}  // extern "C"
