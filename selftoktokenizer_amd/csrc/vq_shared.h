// Pieces of the VQ lookup shared by vq.hip (argmax) and vq_topk.hip (k best codes): the canonical row normalisation, the
// "could make a score non-finite" test and the MFMA-fragment layout of the packed code book.  See vq.hip for the contract.
#pragma once
#include "common.h"

namespace selftok {

constexpr int D = 16;
constexpr uint32_t KEY_NAN = 0xFFFFFFFFu;

// canonical l2norm of one 16-float row (see the header of vq.hip)
__device__ __forceinline__ void l2norm16(const float (&z)[D], float (&x)[D])
{
    float a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = __builtin_fmaf(z[j + 8], z[j + 8], z[j] * z[j]);
    float s = a[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) s = s + a[j];
    float nrm = __builtin_sqrtf(s);   // correctly rounded (refined v_sqrt); __fsqrt_rn is the raw 1-ulp v_sqrt_f32 on gfx950
    nrm = (nrm > 1e-12f) ? nrm : 1e-12f;
    if (s != s) nrm = s;
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = z[k] / nrm;   // IEEE divide (div_scale/div_fmas/div_fixup)
}

__device__ __forceinline__ void load_row16(const float* __restrict__ p, float (&z)[D])
{
    const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float4 t = p4[q];
        z[4 * q + 0] = t.x; z[4 * q + 1] = t.y; z[4 * q + 2] = t.z; z[4 * q + 3] = t.w;
    }
}

// a value that can make a score non-finite: NaN/inf or absurdly large
__device__ __forceinline__ bool suspicious(float v) { return !(fabsf(v) < 1.0e18f); }

typedef float f32x16 __attribute__((ext_vector_type(16)));

// packed layout: tile t (32 codes) = 512 floats = [part 0..1][lane 0..63][4 floats]; lane l = (h = l>>5, i = l&31)
// owns e[t*32+i][2m+h] for m = 4*part + j -- exactly the A fragments of the 8 chained 32x32x2 MFMAs, stored so that
// one wave reads (or DMAs into LDS) a whole 1 KiB (tile, part) piece with 16 B per lane, conflict-free.
__device__ __forceinline__ int packed_offset(int i /*code in tile*/, int k /*element*/)
{
    const int m = k >> 1, lane = (k & 1) * 32 + i;
    return (m >> 2) * 256 + lane * 4 + (m & 3);
}
constexpr int M_CH = 8;                 // code tiles per LDS chunk: 8 x 2 KiB = 16 KiB, double buffered

}  // namespace selftok
