// Device image I/O (include/selftok_hip_ext.h): the two ends of the reference's user script around the tokenizer.
//   in : uint8 HWC images of any sizes -> Resize(S) [Pillow's 8-bit bilinear resample, bit for bit] -> CenterCrop(S) -> lut[u8]
//   out: [B, 3, H, W] in [0, 1] -> uint8 [B, H, W, 3] with save_image's arithmetic in the tensor's own type
// The input end is a special case of a view (csrc/image_views.hip): box = the whole source, resized size = torchvision's Resize(S), window =
// CenterCrop(S), no flip.  This file owns exactly that: how a [B, 3] row (offset, w, h) becomes the descriptor, on the host and again on the
// device, and the entry's error texts.  The resample itself -- limits, workspace, the four kernels, their launch -- is image_resample_shared.h.
// The output end (img_to_u8) is one kernel around the byte rule of u8_shared.h.  Memory-bound and small (tens of MB per batch); the stage is
// bound by the host and the copy.
#include "common.h"
#include "selftok_hip_ext.h"
#include "image_resample_shared.h"
#include "u8_shared.h"
#include <stdio.h>

#pragma clang fp contract(off)

namespace selftok {
namespace {

__host__ __device__ inline int crop_offset(int side, int S)       // int(round((side - S) / 2.0)), Python's round: half to even
{
    const int d = side - S, q = d >> 1;
    return (d & 1) ? q + (q & 1) : q;
}

struct CenterRow {                            // [B, 3]: byte offset, width, height
    static constexpr int COLS = 3, MAX_N = 1 << 30;
    static constexpr const char* WHO = "img_resize_crop_norm";
    static constexpr const char* QUERY = "selftok_img_resize_crop_norm_u8_workspace_bytes";
    static constexpr const char* NEED = "img_resize_crop_norm: need a table, B >= 1 and 1 <= S <= 4096";

    // torchvision Resize(S) on a PIL image + CenterCrop(S): the whole source as the box, the target size, the crop origin as the window
    __host__ __device__ static void describe(const long* r, int S, long* d)
    {
        const long w = r[1], h = r[2];
        long rw = S, rh = S;                  // a side outside 1 .. 65536 is refused by geometry() before it looks at these
        if (w >= 1 && h >= 1 && w <= MAX_SIDE && h <= MAX_SIDE) {
            if (w < h) rh = (long)((double)((long long)S * h) / (double)w);
            else       rw = (long)((double)((long long)S * w) / (double)h);
        }
        d[D_OFF] = r[0]; d[D_W] = w; d[D_H] = h; d[D_X0] = 0; d[D_Y0] = 0; d[D_BW] = w; d[D_BH] = h; d[D_RW] = rw; d[D_RH] = rh;
        d[D_LEFT] = crop_offset((int)rw, S); d[D_TOP] = crop_offset((int)rh, S); d[D_FLIP] = 0;
    }

    static void refuse(int b, int bad, const long* d, int)
    {
        char msg[200];
        if (d[D_W] < 1 || d[D_H] < 1) snprintf(msg, sizeof msg, "img_resize_crop_norm: image %d has a zero side (%ld x %ld)", b, d[D_W], d[D_H]);
        else if (bad == G_BYTES) snprintf(msg, sizeof msg, "img_resize_crop_norm: image %d (offset %ld, %ld x %ld x 3 bytes) reaches past the packed buffer", b, d[D_OFF], d[D_W], d[D_H]);
        else snprintf(msg, sizeof msg, "img_resize_crop_norm: image %d (%ld x %ld) is outside the limits (side <= 65536, resized side < 2^30)", b, d[D_W], d[D_H]);
        set_last_error(msg);
    }
};

template <bool BF16>
__global__ void __launch_bounds__(256) img_to_u8_kernel(const void* __restrict__ img, unsigned char* __restrict__ out, int B, int HW)
{
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)B * HW) return;
    const int b = (int)(p / HW), q = (int)(p % HW);
    const size_t base = (size_t)b * 3 * HW + q;
    unsigned char v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float x = BF16 ? bf16_to_f32(((const unsigned short*)img)[base + (size_t)c * HW]) : ((const float*)img)[base + (size_t)c * HW];
        v[c] = to_u8_one<BF16>(x);
    }
    unsigned char* o = out + (size_t)p * 3;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

size_t selftok_img_resize_crop_norm_u8_workspace_bytes(const long* table_host, int B, int S)
{
    Layout L;
    return plan_host<CenterRow>(table_host, B, S, &L, nullptr) ? L.total : 0;
}

int selftok_img_resize_tables_layout(const long* table_host, int B, int S, long* layout4)
{
    if (!layout4) { set_last_error("img_resize_tables_layout: null output"); return SELFTOK_EINVAL; }
    return tables_layout<CenterRow>(table_host, B, S, layout4);
}

int selftok_img_resize_crop_norm_u8(const unsigned char* packed, size_t packed_bytes, const long* table_host, const long* table_dev, int B, int S, void* out,
                                    int out_bf16, const void* lut, void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    return resample_run<CenterRow>(packed, packed_bytes, table_host, table_dev, B, S, out, out_bf16, lut, workspace, workspace_bytes, stream);
}

int selftok_img_to_u8(const void* img, int in_bf16, unsigned char* out, int B, int H, int W, hipStream_t stream)
{
    if (!img || !out || B < 0 || H < 1 || W < 1 || (long)B * H * W >= (1l << 31)) { set_last_error("img_to_u8: bad argument (need B >= 0, H, W >= 1, B * H * W < 2^31)"); return SELFTOK_EINVAL; }
    if (B == 0) return SELFTOK_OK;
    const long n = (long)B * H * W;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (in_bf16) hipLaunchKernelGGL(img_to_u8_kernel<true>, dim3(blocks), dim3(256), 0, stream, img, out, B, H * W);
    else hipLaunchKernelGGL(img_to_u8_kernel<false>, dim3(blocks), dim3(256), 0, stream, img, out, B, H * W);
    return check_launch("img_to_u8_kernel");
}

}  // extern "C"
