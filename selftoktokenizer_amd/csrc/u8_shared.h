// The byte `save_image` writes for a [0, 1] value, and the bf16 helpers it needs.  The only definition: csrc/image_io.hip (img_to_u8), csrc/image_metrics.hip
// and the input stages of csrc/lpips.hip and csrc/fid.hip all include it.
#pragma once
#include "common.h"

namespace selftok {

__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ float round_bf16(float f)              // fp32 -> nearest bf16 (ties to even), as fp32; not for NaN
{
    unsigned u = __float_as_uint(f);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return __uint_as_float(u & 0xFFFF0000u);
}

// pinned to tests/image_io_cases.py::to_u8_bf16 / to_u8_f32: x * 255, + 0.5, each rounded to the tensor's type, clamp, truncate
template <bool BF16>
__device__ __forceinline__ unsigned char to_u8_one(float x)
{
    if (x != x) return 0;                                         // NaN: this project's choice
    float y = x * 255.0f;
    if (BF16) y = round_bf16(y);
    y = y + 0.5f;
    if (BF16) y = round_bf16(y);
    y = y < 0.0f ? 0.0f : (y > 255.0f ? 255.0f : y);
    return (unsigned char)(int)y;
}

}  // namespace selftok
