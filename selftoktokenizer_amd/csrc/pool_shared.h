// The window pool of channels-last fp32 maps [N, H, W, C] shared by csrc/lpips.hip (3 x 3 / 2), csrc/lpips_vgg.hip (2 x 2 / 2) and csrc/fid.hip (3 x 3:
// max / 2, max / 1 pad 1, average / 1 pad 1): ONE body, one thread per output element, channel fastest.  The rule of record:
//   the taps are walked in (kh, kw) order; a tap outside the image (only with padding) never takes part.
//   max: the first in-image tap initialises m, then v > m || v != v replaces it -- a NaN in a window is the window's result (torch's rule).
//   average: s = +0.0f, s = s + tap for the in-image taps in that order, then s / (float)count with the number of in-image taps as the divisor.
// The result goes to channel co_off + c of an output row of `ldo` floats: a branch of a concatenated map writes its own slice and nothing else.
#pragma once
#include "common.h"
#include <stdio.h>

namespace selftok {
namespace pool {

constexpr int NT = 256;

// output side of a KS-wide window with stride S and padding P, floor mode
template <int KS, int S, int P>
inline int out_side(int in) { return (in + 2 * P - KS) / S + 1; }

template <int KS, int S, int P, bool AVG>
__device__ __forceinline__ void pool_element(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, int PH, int PW, int ldo, int co_off, long total)
{
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    long p = i / C;                                               // output pixel index over the batch
    const long pixel = p;
    const int px = (int)(p % PW); p /= PW;
    const int py = (int)(p % PH);
    const long n = p / PH;
    const int iy0 = py * S - P, ix0 = px * S - P;                 // the window's first tap; outside the image only with padding
    const long org = (((long)n * H + iy0) * W + ix0) * C + c;     // its element index: one address per window, the taps at constant offsets from it
    float m = 0.0f;
    int count = 0;
#pragma unroll
    for (int dy = 0; dy < KS; ++dy)
#pragma unroll
        for (int dx = 0; dx < KS; ++dx) {
            if (P > 0 && (iy0 + dy < 0 || iy0 + dy >= H || ix0 + dx < 0 || ix0 + dx >= W)) continue;      // without padding every window lies inside the image
            const float v = in[org + ((long)dy * W + dx) * C];
            if (AVG) m = m + v;
            else if (count == 0 || v > m || v != v) m = v;
            ++count;
        }
    out[(size_t)pixel * ldo + co_off + c] = AVG ? m / (float)count : m;
}

// the refusals of a pool entry `name`; sets PH x PW and the number of output elements, false with the error set
template <int KS, int S, int P>
inline bool check(const char* name, const float* in, const float* out, int N, int H, int W, int C, int ldo, int co_off, int* PH, int* PW, long* total)
{
    char msg[240];
    constexpr int MIN_SIDE = P > 0 ? 1 : KS;
    constexpr long LIM = 1l << 31;
    if (!in || !out) { snprintf(msg, sizeof msg, "%s: null pointer", name); set_last_error(msg); return false; }
    if (N < 1 || C < 1 || H < MIN_SIDE || W < MIN_SIDE) {
        snprintf(msg, sizeof msg, "%s: need N, C >= 1 and H, W >= %d (one window), got N %d, %d x %d, C %d", name, MIN_SIDE, N, H, W, C); set_last_error(msg); return false;
    }
    if (co_off < 0 || (long)ldo < (long)co_off + C) {
        snprintf(msg, sizeof msg, "%s: the slice needs co_off >= 0 and ldo >= co_off + C, got ldo %d, co_off %d, C %d", name, ldo, co_off, C); set_last_error(msg); return false;
    }
    *PH = out_side<KS, S, P>(H); *PW = out_side<KS, S, P>(W);
    if ((long)H * W >= LIM / C || (long)N >= LIM / ((long)H * W * C) || (long)*PH * *PW >= LIM / ldo || (long)N >= LIM / ((long)*PH * *PW * ldo)) {
        snprintf(msg, sizeof msg, "%s: the input N * H * W * C and the output map must stay below 2^31 elements, got N %d, %d x %d, C %d, ldo %d", name, N, H, W, C, ldo);
        set_last_error(msg); return false;
    }
    *total = (long)N * *PH * *PW * C;
    return true;
}

}  // namespace pool
}  // namespace selftok
