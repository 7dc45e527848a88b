// The fp32 implicit-GEMM convolution on v_mfma_f32_32x32x2_f32 shared by csrc/lpips.hip (selftok_lpips_conv2d_f32) and csrc/fid.hip
// (selftok_fid_conv2d_f32): ONE kernel body, so both entries have the same arithmetic of record, stated at the top of csrc/lpips.hip
// (eight fmaf chains by k mod 16, a fixed fp32 tree, one bias addition, the optional ReLU) and the same packed weight layout
// ([KP][CoutP], row k = (kh * KW + kw) * Cin + ci).  The geometry is general: KH x KW kernel, pad_h / pad_w per axis, and an output row
// of `ldo` floats of which this convolution writes the Cout channels from `co_off` on -- a branch of a concatenated map writes its own
// slice and nothing else.  The LPIPS entry passes pad_h = pad_w, ldo = Cout, co_off = 0.  The host side of both entries is conv_plan below.
#pragma once
#include "common.h"
#include <stdio.h>

namespace selftok {
namespace conv_f32 {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 64, BN = 64, KT = 16, LDS_STRIDE = 68, NT = 256;

struct ConvArgs {
    const float* in; const float* wp; const float* bias; float* out;
    int H, W, Cin, OH, OW, Cout, CoutP, KH, KW, stride, pad_h, pad_w, K, KP, relu, ldo, co_off;
    long M;
};

// the tap walk of one gather lane: k -> (kh, kw, ci), advanced without a division
struct Tap {
    int kh, kw, ci;
    __device__ __forceinline__ void advance(int by, int Cin, int KW)
    {
        ci += by;
        while (ci >= Cin) { ci -= Cin; if (++kw == KW) { kw = 0; ++kh; } }
    }
};

// one workgroup (256 threads, 4 waves) = one 64 x 64 tile of the [M, Cout] output; grid (ceil(M / 64), CoutP / 64)
template <bool VEC>
__device__ __forceinline__ void conv_tile(const ConvArgs& a)
{
    __shared__ __attribute__((aligned(16))) float As[KT * LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) float Bs[KT * LDS_STRIDE];   // written as float4: bk * 68 + bc is a multiple of 4
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long m0 = (long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;

    // gather role: row ar of the tile, taps akq .. akq + 3 of every step
    const int ar = tid >> 2, akq = (tid & 3) * 4;
    const long am = m0 + ar;
    const bool arow = am < a.M;
    int iy0 = 0, ix0 = 0;
    const float* aimg = a.in;
    if (arow) {
        const long per = (long)a.OH * a.OW;
        const long n = am / per;
        const int rem = (int)(am - n * per);
        const int oy = rem / a.OW, ox = rem - oy * a.OW;
        iy0 = oy * a.stride - a.pad_h; ix0 = ox * a.stride - a.pad_w;
        aimg = a.in + (size_t)n * a.H * a.W * a.Cin;
    }
    Tap tap{0, 0, 0};
    tap.advance(akq, a.Cin, a.KW);
    // weight role: row bk of the step, columns bc .. bc + 3
    const int bk = tid >> 4, bc = (tid & 15) * 4;
    const float* bsrc = a.wp + (size_t)bk * a.CoutP + n0 + bc;

    float4 areg, breg;
    auto fetch = [&](int k0) {
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (VEC) {
            if (arow && k0 + akq < a.K) {
                const int iy = iy0 + tap.kh, ix = ix0 + tap.kw;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                    const float4 q = *(const float4*)(aimg + ((size_t)iy * a.W + ix) * a.Cin + tap.ci);
                    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                }
            }
        } else {
            Tap t = tap;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (arow && k0 + akq + j < a.K) {
                    const int iy = iy0 + t.kh, ix = ix0 + t.kw;
                    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v[j] = aimg[((size_t)iy * a.W + ix) * a.Cin + t.ci];
                }
                t.advance(1, a.Cin, a.KW);
            }
        }
        areg = make_float4(v[0], v[1], v[2], v[3]);
        breg = *(const float4*)(bsrc + (size_t)k0 * a.CoutP);
        tap.advance(KT, a.Cin, a.KW);
    };

    f32x16 acc[KT / 2];                                           // chain j = acc[j]
#pragma unroll
    for (int j = 0; j < KT / 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    const int fr = lane & 31, fk = lane >> 5;

    fetch(0);
    for (int k0 = 0; k0 < a.KP; k0 += KT) {
        __syncthreads();                                          // the previous step's MFMA reads are done
        As[(akq + 0) * LDS_STRIDE + ar] = areg.x; As[(akq + 1) * LDS_STRIDE + ar] = areg.y;
        As[(akq + 2) * LDS_STRIDE + ar] = areg.z; As[(akq + 3) * LDS_STRIDE + ar] = areg.w;
        *(float4*)(Bs + bk * LDS_STRIDE + bc) = breg;
        __syncthreads();
        if (k0 + KT < a.KP) fetch(k0 + KT);                       // in flight while the MFMAs below run
#pragma unroll
        for (int kk = 0; kk < KT; kk += 2) {                      // taps kk, kk + 1 of this step -> chain kk / 2
            const float av = As[(kk + fk) * LDS_STRIDE + wm + fr];
            const float bv = Bs[(kk + fk) * LDS_STRIDE + wn + fr];
            acc[kk / 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[kk / 2], 0, 0, 0);
        }
    }
    const f32x16 sum = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));

    const int co = n0 + wn + fr;
    if (co >= a.Cout) return;
    const float bias = a.bias ? a.bias[co] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * fk;
        if (m >= a.M) continue;
        float v = a.bias ? sum[r] + bias : sum[r];
        if (a.relu) v = v < 0.0f ? 0.0f : v;
        a.out[(size_t)m * a.ldo + a.co_off + co] = v;
    }
}

// output side of a convolution / pool, 0 when there is no output pixel
inline int out_side(int in, int k, int stride, int pad) { const long s = (long)in + 2l * pad - k; return s < 0 ? 0 : (int)(s / stride + 1); }

// the host side of a convolution entry `name` (its name in the messages): every refusal -- geometry, slice, the element counts of input, output map
// and packed weight below 2^31, alignment, the grid limit -- then the ConvArgs and the grid of its `*_conv_kernel<VEC>`, VEC = (Cin % 4 == 0).
// false with the error set.
inline bool conv_plan(const char* name, const float* in, const float* packed, const float* bias, float* out, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                      int stride, int pad_h, int pad_w, int ldo, int co_off, int relu, ConvArgs* a, dim3* grid)
{
    char msg[320];
    auto fail = [&] { set_last_error(msg); return false; };
    constexpr long LIM = 1l << 31;
    if (!in || !packed || !out) { snprintf(msg, sizeof msg, "%s: null pointer", name); return fail(); }
    if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || KH < 1 || KW < 1 || stride < 1 || pad_h < 0 || pad_h >= KH || pad_w < 0 || pad_w >= KW) {
        snprintf(msg, sizeof msg, "%s: need N, H, W, Cin, Cout, KH, KW, stride >= 1, 0 <= pad_h < KH and 0 <= pad_w < KW, got N %d, %d x %d, Cin %d, Cout %d, "
                 "%d x %d, stride %d, pad %d, %d", name, N, H, W, Cin, Cout, KH, KW, stride, pad_h, pad_w);
        return fail();
    }
    if (co_off < 0 || (long)ldo < (long)co_off + Cout) {
        snprintf(msg, sizeof msg, "%s: the slice needs co_off >= 0 and ldo >= co_off + Cout, got ldo %d, co_off %d, Cout %d", name, ldo, co_off, Cout);
        return fail();
    }
    const int OH = out_side(H, KH, stride, pad_h), OW = out_side(W, KW, stride, pad_w);
    if (OH < 1 || OW < 1) {
        snprintf(msg, sizeof msg, "%s: %d x %d input has no output pixel under a %d x %d kernel with pad %d, %d", name, H, W, KH, KW, pad_h, pad_w);
        return fail();
    }
    const long kk = (long)KH * KW;
    if (kk >= LIM / Cin || (long)H * W >= LIM / Cin || (long)N >= LIM / ((long)H * W * Cin) || (long)OH * OW >= LIM / ldo ||
        (long)N >= LIM / ((long)OH * OW * ldo) || ((kk * Cin + KT - 1) / KT * KT) >= LIM / ((Cout + BN - 1) / BN * BN)) {
        snprintf(msg, sizeof msg, "%s: input, output map and packed weight element counts must stay below 2^31, got N %d, %d x %d, Cin %d, Cout %d, %d x %d, ldo %d",
                 name, N, H, W, Cin, Cout, KH, KW, ldo);
        return fail();
    }
    if (((uintptr_t)in & 15) != 0 || ((uintptr_t)packed & 15) != 0 || ((uintptr_t)out & 3) != 0 || ((uintptr_t)bias & 3) != 0) {
        snprintf(msg, sizeof msg, "%s: in and packed must be 16-byte aligned, out and bias 4-byte aligned", name); return fail();
    }
    *a = ConvArgs{in, packed, bias, out, H, W, Cin, OH, OW, Cout, (Cout + BN - 1) / BN * BN, KH, KW, stride, pad_h, pad_w, KH * KW * Cin,
                  (KH * KW * Cin + KT - 1) / KT * KT, relu != 0, ldo, co_off, (long)N * OH * OW};
    *grid = dim3((unsigned)((a->M + BM - 1) / BM), (unsigned)(a->CoutP / BN));
    if (grid->y > 65535u) { snprintf(msg, sizeof msg, "%s: Cout above 64 * 65535", name); return fail(); }
    return true;
}

}  // namespace conv_f32
}  // namespace selftok
