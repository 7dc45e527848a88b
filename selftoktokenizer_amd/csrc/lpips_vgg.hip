// The one stage LPIPS on the VGG16 backbone needs beyond csrc/lpips.hip (include/selftok_hip_ext.h): the 2 x 2 stride 2 max-pool of torchvision's
// VGG16 `features` (MaxPool2d(2, 2), floor mode: the last row / column of an odd map is dropped), an instance of csrc/pool_shared.h's body.  The 13
// convolutions run on selftok_lpips_conv2d_f32, the input and distance stages are lpips.hip's; selftoktokenizer_amd/lpips.py (LPIPS_VGG_DEFINITION) chains them.
// Activations are channels-last fp32 [N, H, W, C].  It is a file of its own so that lpips.hip's kernels stay the nine its budget is stated for.
#include "common.h"
#include "pool_shared.h"
#include "selftok_hip_ext.h"

namespace selftok {
namespace {

using pool::NT;

// every window lies inside the image.  A NaN wins (torch's rule), as in the 3 x 3 pool.
__global__ void __launch_bounds__(NT) lpips_pool2_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, int PH, int PW, long total)
{
    pool::pool_element<2, 2, 0, false>(in, out, H, W, C, PH, PW, C, 0, total);
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

int selftok_lpips_maxpool2s2_f32(const float* in, float* out, int N, int H, int W, int C, hipStream_t stream)
{
    int PH, PW;
    long total;
    if (!pool::check<2, 2, 0>("lpips_maxpool2s2", in, out, N, H, W, C, C, 0, &PH, &PW, &total)) return SELFTOK_EINVAL;
    hipLaunchKernelGGL(lpips_pool2_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, stream, in, out, H, W, C, PH, PW, total);
    return check_launch("lpips_pool2_kernel");
}

}  // extern "C"
