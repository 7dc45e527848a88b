// The byte `save_image` writes for a [0, 1] value, the bf16 helpers it needs, and the pixel conversion of the evaluation entries (load, unit range, byte).
// The only definition: csrc/image_io.hip (img_to_u8), csrc/image_metrics.hip, csrc/image_ssim.hip and the input stages of csrc/lpips.hip and csrc/fid.hip
// all include it.  Plain C++ around the intrinsics tests/host_standin/common.h defines: a host compiler builds it.
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

// element `at` of a bf16 (BF) or fp32 tensor, as fp32
template <bool BF>
__device__ __forceinline__ float load_px(const void* t, size_t at)
{
    return BF ? bf16_to_f32(((const unsigned short*)t)[at]) : ((const float*)t)[at];
}

// o in [0, 1] of a pixel v: evaluate.psnr_each's fp32 expression for a [-1, 1] image, a [0, 1] image as it is
__device__ __forceinline__ float px_unit(float v, bool is_signed) { return is_signed ? (v + 1.0f) / 2.0f : v; }

// the byte of a pixel: to_u8_one of its unit value, rounded in the type ROUND_BF16 names -- chosen by the caller, because the entries differ ON PURPOSE:
// lpips_input, img_metrics and img_ssim quantize the reconstruction in its own type and the ORIGINAL in fp32 (<false>) whatever its dtype (o is an fp32
// value even when v was bf16); fid_input quantizes an unsigned image in its own type (<BF>) and a signed one in fp32.  For an unsigned bf16 original these
// are different bytes, and each is the one its emulation (tests/image_metrics_cases.py, tests/lpips_cases.py, tests/fid_cases.py) pins.
template <bool ROUND_BF16>
__device__ __forceinline__ unsigned char px_u8(float v, bool is_signed) { return to_u8_one<ROUND_BF16>(px_unit(v, is_signed)); }

}  // namespace selftok
