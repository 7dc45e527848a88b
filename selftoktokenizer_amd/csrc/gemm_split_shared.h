// What the Linear kernels on the split planes share (gemm_split.hip: the f16x2 kernels; gemm_f16.hip: the single-pass fp16 kernel
// on the same operands): tile shape, the packed weight image, the work-group -> tile map, the fp32 -> (hi, lo) split, the GELU, the
// LDS-DMA piece, the arguments of the fused residual epilogue and, for the host, the argument contract of the split-input entry points.
// One definition each, so that "the same operations in the same order" is the same code.
#pragma once
#include "common.h"
#include <stdio.h>

namespace selftok {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16v __attribute__((ext_vector_type(16)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

constexpr int BM = 256, BN = 128, BK = 32;
constexpr float LO_SCALE = 2048.0f, LO_INV = 1.0f / 2048.0f;
constexpr float F16_MAX = 65504.0f;

constexpr int W_G = BN * 16;               // weight image: linear (filled by LDS-DMA)
constexpr int W_P = 4 * W_G;
constexpr int W_BYTES = 2 * W_P;           // 16384
constexpr int GROUP_M = 4;                 // 32 consecutive tiles (one XCD's resident set) = 4 row blocks x 8 column blocks

// tile id of a work-group: XCD-contiguous renumbering (bijective), then grouped-M walk.  Work-groups are renumbered so that each
// XCD (own L2) owns a contiguous range of tiles, walked in groups of GROUP_M row blocks, which keeps the A row panels and W column
// panels of concurrently running work-groups in one L2.  One work-group per tile: gridDim.x = mblocks * nblocks.
__device__ __forceinline__ void tile_of_workgroup(int mblocks, int nblocks, int& mb, int& nb)
{
    const int T = gridDim.x, orig = blockIdx.x;
    const int q8 = T >> 3, r8 = T & 7, xcd = orig & 7, idx = orig >> 3;
    const int w = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    const int per_group = GROUP_M * nblocks;
    const int group = w / per_group, first_m = group * GROUP_M;
    const int gsz = (mblocks - first_m) < GROUP_M ? (mblocks - first_m) : GROUP_M;
    const int in = w - group * per_group;
    mb = first_m + in % gsz;
    nb = in / gsz;
}

// GELU(tanh): 0.5 x (1 + tanh(u)) = x sigmoid(2u) = x / (1 + exp(-2u)), u = sqrt(2/pi) (x + 0.044715 x^3).  The sigmoid form needs one
// v_exp_f32 + one v_rcp_f32 (1 ulp each) instead of ocml's tanhf (~40 VALU ops: the GELU epilogue was 8 % of the fc1 kernel) and has no
// cancellation in 1 + tanh(u) for negative x; |error| vs the fp64 GELU stays below the tanhf form's (tests/test_gemm_gpu.py).
// -inf -> NaN and +inf -> +inf as the reference formula gives.
__device__ __forceinline__ float gelu_tanh_f(float x)
{
    const float k0 = 0.7978845608028654f, k1 = 0.044715f;
    const float u = k0 * (x + k1 * x * x * x);
    const float e = __builtin_amdgcn_exp2f(u * (-2.0f * 1.4426950408889634f));
    return x * __builtin_amdgcn_rcpf(1.0f + e);
}

typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// four fp32 -> four (hi, lo) fp16 pairs, written with 2-wide vectors so that the residual and its 2^11 scaling are packed
// VALU ops (v_pk_add_f32 / v_pk_mul_f32): a wave64 VALU instruction occupies its SIMD for 8 cycles, and with two waves per SIMD
// the split would otherwise keep the VALU pipe as busy as the matrix pipe.  `mx` (optional) tracks max |x| for the range check.
template <typename V4>
__device__ __forceinline__ void split4(const V4& v, f16x4& hi, f16x4& lo)
{
    // __builtin_convertvector keeps the pair packed: v_cvt_pk_f16_f32, v_cvt_f32_f16 (+ one SDWA form for the upper half),
    // v_pk_add_f32, v_pk_mul_f32, v_cvt_pk_f16_f32 = 3 VALU ops per element (element-wise casts compile to 4.5)
    const f32x2v a = {v.x, v.y}, b = {v.z, v.w};
    const f16x2 ha = __builtin_convertvector(a, f16x2), hb = __builtin_convertvector(b, f16x2);
    const f32x2v ra = (a - __builtin_convertvector(ha, f32x2v)) * LO_SCALE;                        // exact residual, then 2^11
    const f32x2v rb = (b - __builtin_convertvector(hb, f32x2v)) * LO_SCALE;
    const f16x2 la = __builtin_convertvector(ra, f16x2), lb = __builtin_convertvector(rb, f16x2);
    hi[0] = ha[0]; hi[1] = ha[1]; hi[2] = hb[0]; hi[3] = hb[1];
    lo[0] = la[0]; lo[1] = la[1]; lo[2] = lb[0]; lo[3] = lb[1];
}
template <typename V4>
__device__ __forceinline__ void split4(const V4& v, f16x4& hi, f16x4& lo, float& mx)
{
    split4(v, hi, lo);
    mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
}

// LDS image of a pre-split activation tile (see linear_f16x2_pre_kernel): [plane][row 0..255][4 slots of 16 B]
constexpr int PA_ROW = 64;                       // bytes per row and plane of a 32-deep k-tile
constexpr int PA_P = BM * PA_ROW;                // 16384

// one LDS-DMA piece: 64 lanes x 16 B from (uniform base + per-lane 32-bit byte offset) to LDS [lds, lds + 1 KiB) in lane order.
// Inline asm because hipcc will not select the SGPR-base form for the builtin (it rebuilds a 64-bit VGPR address per piece).
__device__ __forceinline__ void lds_dma16(const void* base, unsigned voff, unsigned lds)
{
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(base), "s"(lds) : "memory", "m0");   // M0 declared as clobbered
}

// fused residual epilogue (RES): out = resid + gate * (A W^T + bias), gate element (row, col) at gate + (row / T) gsb + (row % T) gst + col
// (per-sample table: gst = 0; per-token table: gsb = 0; gate NULL: out = resid + y).  The multiply and the add are separate
// fp32 operations, exactly as residual_ln_mod_kernel performs them on the stored y: same bits, one tensor round trip less.
struct ResArgs { const float* resid; long ldr; const float* gate; long gsb, gst; int T; };

// ---- host: the argument contract of the entry points that take a split activation (selftok_linear_f16x2_split, ..._split_k,
// selftok_linear_f16_split and their _residual forms), `who` = the entry's name for the message.  Order of decisions: a bad shape is
// refused; then M == 0 is SELFTOK_OK without a look at the pointers; then pointers, alignment and strides.  The caller returns the
// result if it is not SELFTOK_OK or if M == 0, and launches otherwise.
inline int refuse_args(const char* who, const char* what)
{
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    set_last_error(msg);
    return SELFTOK_EINVAL;
}

inline int check_split_linear(const char* who, const void* a_blk, const void* packed, const float* bias, const float* out, const void* out_blk,
                              long ldo, int M, int N, int K)
{
    if (M < 0 || N <= 0 || K <= 0 || N % BN || K % BK) return refuse_args(who, "need N % 128 == 0 and K % 32 == 0");
    if (M == 0) return SELFTOK_OK;
    if (!a_blk || !packed || ((size_t)a_blk & 15) || ((size_t)out & 15) || ((size_t)out_blk & 15) || (bias && ((size_t)bias & 15))
        || (out_blk ? out != nullptr : (!out || ldo < N || (ldo & 3))))
        return refuse_args(who, "bad pointers/strides (a_blk, out, out_blk and bias 16-byte aligned; either out with ldo % 4 == 0, ldo >= N, or out_blk)");
    return SELFTOK_OK;
}

inline int check_split_linear_residual(const char* who, const void* a_blk, const void* packed, const float* bias, const float* resid, long ldr,
                                       const float* gate, long gate_stride_b, long gate_stride_t, int T, const float* out, long ldo,
                                       int M, int N, int K)
{
    if (int rc = check_split_linear(who, a_blk, packed, bias, out, nullptr, ldo, M, N, K)) return rc;
    if (M == 0) return SELFTOK_OK;
    if (!resid || ldr < N || (ldr & 3) || T <= 0 || ((size_t)resid & 15)
        || (gate && (((size_t)gate & 15) || (gate_stride_b & 3) || (gate_stride_t & 3))))
        return refuse_args(who, "bad residual arguments (resid and gate 16-byte aligned, ldr >= N, ldr and the gate strides multiples of 4, T > 0)");
    return SELFTOK_OK;
}

// split-K (the f16x2 and f16 _k entries): 2 .. 64 parts, each a whole number of k-tiles, and a workspace to put them in
inline int check_splitk(const char* who, int K, int ksplit, const void* workspace)
{
    if (ksplit >= 2 && ksplit <= 64 && (K / BK) % ksplit == 0 && workspace && !((size_t)workspace & 15)) return SELFTOK_OK;
    return refuse_args(who, "ksplit not in 2..64 / not a divisor of K / 32, or no 16-byte aligned workspace");
}

// second launch of every split-K Linear (defined in gemm_split.hip, next to splitk_finish_kernel): out = epilogue(sum of the `ksplit` planes
// [M][N] of `ws` in ascending order + bias).  `res` == nullptr: flags (SELFTOK_LINEAR_GELU) and fp32 `out` or the split output `out_blk`;
// otherwise the fused residual update into `out`.  Arguments already checked by the entry.
int launch_splitk_finish(const float* ws, int ksplit, const float* bias, float* out, void* out_blk, long ldo, int M, int N, int flags,
                         int* overflow, const ResArgs* res, hipStream_t stream);

}  // namespace selftok
