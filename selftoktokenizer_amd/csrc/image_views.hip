// Device image views (include/selftok_hip_ext.h): V outputs of S x S taken from packed uint8 HWC sources, each by a descriptor row
//   crop(x0, y0, bw, bh) -> resize to Rw x Rh [Pillow's 8-bit bilinear resample, each axis on its own] -> window (left, top, S, S) -> flip -> lut[u8]
// which is torchvision's five / ten-crop, resized_crop and hflip on a PIL image, bit for bit.  The [V, 12] rows are the descriptor of
// image_resample_shared.h as they are, so this file owns only the row type and the entry's error texts; the limits, the workspace, the four
// kernels and their launch are the header's, shared with the centre-crop entry of csrc/image_io.hip.
#include "common.h"
#include "selftok_hip_ext.h"
#include "image_resample_shared.h"
#include <stdio.h>

#pragma clang fp contract(off)

namespace selftok {
namespace {

struct ViewRow {                              // [V, 12]: the descriptor itself
    static constexpr int COLS = NV, MAX_N = MAX_OUTPUTS;
    static constexpr const char* WHO = "img_views";
    static constexpr const char* QUERY = "selftok_img_views_u8_workspace_bytes";
    static constexpr const char* NEED = "img_views: need a view table, 1 <= V <= 65535 and 1 <= S <= 4096";

    __host__ __device__ static void describe(const long* r, int, long* d)
    {
        for (int i = 0; i < NV; ++i) d[i] = r[i];
    }

    static void refuse(int v, int bad, const long* d, int S)
    {
        static const char* const why[] = {"", "a source side outside 1 .. 65536", "a box that is empty or outside the source", "a resized side below S or >= 2^30",
                                          "a window outside the resized box", "a flip that is neither 0 nor 1", "no box row under its window"};
        char msg[256];
        if (bad == G_BYTES) snprintf(msg, sizeof msg, "img_views: the source of view %d (offset %ld, %ld x %ld x 3 bytes) reaches past the packed buffer", v, d[D_OFF], d[D_W], d[D_H]);
        else snprintf(msg, sizeof msg, "img_views: view %d has %s (source %ld x %ld, box %ld,%ld %ld x %ld -> %ld x %ld, window %ld,%ld, S %d, flip %ld)", v, why[bad],
                      d[D_W], d[D_H], d[D_X0], d[D_Y0], d[D_BW], d[D_BH], d[D_RW], d[D_RH], d[D_LEFT], d[D_TOP], S, d[D_FLIP]);
        set_last_error(msg);
    }
};

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

size_t selftok_img_views_u8_workspace_bytes(const long* views_host, int V, int S)
{
    Layout L;
    return plan_host<ViewRow>(views_host, V, S, &L, nullptr) ? L.total : 0;
}

int selftok_img_views_tables_layout(const long* views_host, int V, int S, long* layout4)
{
    if (!layout4) { set_last_error("img_views_tables_layout: null output"); return SELFTOK_EINVAL; }
    return tables_layout<ViewRow>(views_host, V, S, layout4);
}

int selftok_img_views_u8(const unsigned char* packed, size_t packed_bytes, const long* views_host, const long* views_dev, int V, int S, void* out, int out_bf16,
                         const void* lut, void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    return resample_run<ViewRow>(packed, packed_bytes, views_host, views_dev, V, S, out, out_bf16, lut, workspace, workspace_bytes, stream);
}

}  // extern "C"
