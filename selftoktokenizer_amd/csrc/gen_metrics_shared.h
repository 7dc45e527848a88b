// The pair arithmetic of csrc/gen_metrics.hip (selftok_knn_radius_f32 and selftok_manifold_member_f32), written ONCE: both entries run the
// same norm chain, the same dot-product tile loop and the same combination, so the bits of d2(u, v) are a function of the two rows alone.
//
// Arithmetic of record, u and v fp32 rows of length D (a multiple of 16):
//   norm(u)   = (float)n_D,  n_0 = +0.0,  n_{k+1} = fma((double)u_k, (double)u_k, n_k)  (one fp64 chain, k ascending, rounded to fp32 ONCE: the
//               norms cost one pass over the rows, so they are taken accurately and the error of d2 is the dot product's)
//   dot(u, v) = c_D,  c_0 = +0.0f,  c_{k+1} = fmaf(u_k, v_k, c_k)                      (one fmaf chain, k ascending: v_mfma_f32_32x32x2_f32 takes
//               k = 2m in its lanes 0-31 and k = 2m + 1 in its lanes 32-63 and adds them to the accumulator in that order)
//   d2(u, v)  = s - t,  s = norm(u) + norm(v),  t = 2.0f * dot(u, v)  (exact),  then  d2 <= 0 ? +0.0f : d2   (a NaN stays a NaN)
// Every operation is rounded to fp32 on its own (the file is compiled with -ffp-contract=off).  fmaf(a, b, c) = fmaf(b, a, c) and s is a
// commutative sum, so d2(u, v) = d2(v, u) bit for bit, whichever of the two is the matrix instruction's A operand; an output element of the
// matrix instruction depends on its own row and column alone, so neither the tile a pair falls into, nor the rows around it (zero-filled
// rows past the end included), nor the column split changes a bit.
// Error against the real number: |d2 - |u - v|^2| <= (D + 5) * 2^-24 * (|u|^2 + |v|^2).
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace selftok {
namespace gm {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BT = 128;                                           // tile side: 128 lane-side rows x 128 register-side candidates per workgroup
constexpr int KT = 16;                                            // depth of one staged step
constexpr int LDS_STRIDE = BT + 4;                                // [k][row] with a 4-float skew: a wave half reads 32 consecutive floats
constexpr int NT = 256;

__device__ __forceinline__ float row_norm(const float* __restrict__ x, int D)
{
    double n = 0.0;
    for (int k = 0; k < D; k += 4) {
        const float4 q = *(const float4*)(x + k);
        n = fma((double)q.x, (double)q.x, n); n = fma((double)q.y, (double)q.y, n); n = fma((double)q.z, (double)q.z, n); n = fma((double)q.w, (double)q.w, n);
    }
    return (float)n;
}

__device__ __forceinline__ float pair_d2(float norm_u, float norm_v, float dot)
{
    const float s = norm_u + norm_v;
    const float t = 2.0f * dot;
    const float d = s - t;
    return d <= 0.0f ? 0.0f : d;
}

// index inside a 32 x 32 matrix-instruction tile of accumulator register r of lane half fk (rows of the A operand)
__device__ __forceinline__ int acc_row(int r, int fk) { return (r & 3) + 8 * (r >> 2) + 4 * fk; }

// acc[ci][ri][r] = dot(candidate c0 + cm + 32 ci + acc_row(r, fk), row r0 + rm + 32 ri + (lane & 31)) for this wave's 64 x 64 quarter
// (rm = 64 * (wave & 1), cm = 64 * (wave >> 1)) of the 128 x 128 tile.  Rows / candidates past NR / NC are staged as zeros and never read.
// Rs / Cs: KT * LDS_STRIDE floats each.  Every thread of the workgroup must call it (barriers inside).
__device__ __forceinline__ void tile_dots(const float* __restrict__ R, long r0, int NR, const float* __restrict__ Cm, long c0, int NC, int D,
                                          float* Rs, float* Cs, f32x16 (&acc)[2][2])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = tid >> 2, kq = (tid & 3) * 4;                  // loader role: rows lr and lr + 64 of both sides, k = kq .. kq + 3 of every step
    const float* rp[2];
    const float* cp[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const long rr = r0 + lr + 64 * h, cc = c0 + lr + 64 * h;
        rp[h] = rr < NR ? R + (size_t)rr * D + kq : nullptr;
        cp[h] = cc < NC ? Cm + (size_t)cc * D + kq : nullptr;
    }
    float4 rreg[2], creg[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            rreg[h] = rp[h] ? *(const float4*)(rp[h] + k0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            creg[h] = cp[h] ? *(const float4*)(cp[h] + k0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    };
#pragma unroll
    for (int ci = 0; ci < 2; ++ci)
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[ci][ri][i] = 0.0f;
    const int rm = (wave & 1) * 64, cm = (wave >> 1) * 64;
    const int fr = lane & 31, fk = lane >> 5;

    fetch(0);
    for (int k0 = 0; k0 < D; k0 += KT) {
        __syncthreads();                                          // the previous step's (and the previous tile's) LDS reads are done
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int at = kq * LDS_STRIDE + lr + 64 * h;
            Rs[at] = rreg[h].x; Rs[at + LDS_STRIDE] = rreg[h].y; Rs[at + 2 * LDS_STRIDE] = rreg[h].z; Rs[at + 3 * LDS_STRIDE] = rreg[h].w;
            Cs[at] = creg[h].x; Cs[at + LDS_STRIDE] = creg[h].y; Cs[at + 2 * LDS_STRIDE] = creg[h].z; Cs[at + 3 * LDS_STRIDE] = creg[h].w;
        }
        __syncthreads();
        if (k0 + KT < D) fetch(k0 + KT);                          // in flight while the matrix instructions below run
#pragma unroll
        for (int kk = 0; kk < KT; kk += 2) {                      // k0 + kk (lanes 0-31) and k0 + kk + 1 (lanes 32-63): the chain stays k-ascending
            const float* cs = Cs + (kk + fk) * LDS_STRIDE + cm + fr;
            const float* rs = Rs + (kk + fk) * LDS_STRIDE + rm + fr;
            const float a0 = cs[0], a1 = cs[32], b0 = rs[0], b1 = rs[32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
}

}  // namespace gm
}  // namespace selftok
