// The one stage LPIPS on the VGG16 backbone needs beyond csrc/lpips.hip (include/selftok_hip_ext.h): the 2 x 2 stride 2 max-pool of torchvision's
// VGG16 `features` (MaxPool2d(2, 2), floor mode: the last row / column of an odd map is dropped).  The 13 convolutions run on
// selftok_lpips_conv2d_f32, the input and distance stages are lpips.hip's; selftoktokenizer_amd/lpips.py (LPIPS_VGG_DEFINITION) chains them.
// Activations are channels-last fp32 [N, H, W, C].  It is a file of its own so that lpips.hip's kernels stay the nine its budget is stated for.
#include "common.h"
#include "selftok_hip_ext.h"
#include <stdio.h>

namespace selftok {
namespace {

constexpr int NT = 256;

// one thread per output element, channel fastest: every window lies inside the image.  A NaN wins (torch's rule), as in the 3 x 3 pool.
__global__ void __launch_bounds__(NT) lpips_pool2_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, int PH, int PW, long total)
{
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    long p = i / C;
    const int px = (int)(p % PW); p /= PW;
    const int py = (int)(p % PH);
    const long n = p / PH;
    const float* src = in + (((size_t)n * H + 2 * py) * W + 2 * px) * C + c;
    float m = src[0];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const float v = src[((size_t)dy * W + dx) * C];
            if (v > m || v != v) m = v;
        }
    out[i] = m;
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

int selftok_lpips_maxpool2s2_f32(const float* in, float* out, int N, int H, int W, int C, hipStream_t stream)
{
    if (!in || !out) { set_last_error("lpips_maxpool2s2: null pointer"); return SELFTOK_EINVAL; }
    char msg[200];
    if (N < 1 || C < 1 || H < 2 || W < 2) {
        snprintf(msg, sizeof msg, "lpips_maxpool2s2: need N, C >= 1 and H, W >= 2 (one window), got N %d, %d x %d, C %d", N, H, W, C); set_last_error(msg); return SELFTOK_EINVAL;
    }
    const long lim = 1l << 31;
    if ((long)H * W >= lim / C || (long)N >= lim / ((long)H * W * C)) {
        snprintf(msg, sizeof msg, "lpips_maxpool2s2: N * H * W * C must stay below 2^31, got N %d, %d x %d, C %d", N, H, W, C); set_last_error(msg); return SELFTOK_EINVAL;
    }
    const int PH = H / 2, PW = W / 2;
    const long total = (long)N * PH * PW * C;
    hipLaunchKernelGGL(lpips_pool2_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, stream, in, out, H, W, C, PH, PW, total);
    return check_launch("lpips_pool2_kernel");
}

}  // extern "C"
