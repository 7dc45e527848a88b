// The sampler's per-code arithmetic (include/selftok_hip_ext.h, token sampler, steps 1 - 4 and the Philox of step 7), shared by csrc/token_sample.hip and
// csrc/token_verify.hip so that the two kernels can be held to each other by equality: wave shuffles of uint64, the bf16 widening, guidance and temperature in
// four roundings, the orderable key, the integer mass and Philox4x32-10.  Leaf functions only, all forced inline; a kernel's row walk and selects stay in its file.
#pragma once
#include "common.h"

namespace selftok {
namespace tokshared {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned short u16;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

constexpr u32 KEY_NEG_INF = 0x007FFFFFu;                          // f32_orderable(-inf)

__device__ __forceinline__ u64 shfl_u64(u64 v, int src)
{
    const u32 lo = __shfl((u32)v, src, WAVE), hi = __shfl((u32)(v >> 32), src, WAVE);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_up_u64(u64 v, int o)
{
    const u32 lo = __shfl_up((u32)v, o, WAVE), hi = __shfl_up((u32)(v >> 32), o, WAVE);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int o)
{
    const u32 lo = __shfl_xor((u32)v, o, WAVE), hi = __shfl_xor((u32)(v >> 32), o, WAVE);
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ float widen(u16 h) { return __uint_as_float((u32)h << 16); }

// guidance and temperature: difference, product, sum, product -- four roundings, none fused
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

// the monotone uint32 key of a logit (-0.0 as +0.0); a NaN or +inf sets badf
__device__ __forceinline__ u32 key_of(float l, u32& badf)
{
    u32 u = __float_as_uint(l);
    if ((u & 0x7FFFFFFFu) == 0u) u = 0u;                          // -0.0 counts as +0.0
    badf |= ((u & 0x7FFFFFFFu) > 0x7F800000u || u == 0x7F800000u) ? 1u : 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the integer mass of a code d = l - m below the row maximum: trunc(exp(d) * 2^32), exp by n = rint(d * log2 e), a two-constant reduction and a degree-6
// polynomial in separate fp32 multiplies and adds; exactly 2^32 at d = 0, 0 below -24 (and for -inf)
__device__ __forceinline__ u64 mass_of(u32 key, float m)
{
    const float d = f32_from_orderable(key) - m;
    if (!(d >= -24.0f)) return 0ull;
    const float n = rintf(d * 1.4426950408889634f);
    const float r = (d - n * 0.693145751953125f) - n * 1.428606765330187045e-06f;
    float p = (float)(1.0 / 720.0) * r + (float)(1.0 / 120.0);    // the constants rounded to fp32
    p = p * r + (float)(1.0 / 24.0);
    p = p * r + (float)(1.0 / 6.0);
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    const float scale = __uint_as_float((u32)((int)n + 32 + 127) << 23);      // 2^(n + 32), n + 32 in [-3, 32]: the product is exact
    return (u64)(p * scale);
}

__device__ __forceinline__ void philox4x32_10(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1, u32& o0, u32& o1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u32 hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const u32 hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o0 = c0; o1 = c1;
}

}  // namespace tokshared
}  // namespace selftok
