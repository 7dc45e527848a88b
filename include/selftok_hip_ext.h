/*
 * selftok_hip_ext.h -- entry points of libselftok_hip.so that have no CPU twin yet (oracle/libselftok_cpu.so exports
 * exactly the names of selftok_hip.h).  Same conventions as selftok_hip.h: device pointers owned by the caller, explicit
 * sizes, 0 / SELFTOK_EINVAL / SELFTOK_EHIP, nothing allocates, synchronises or keeps state, graph-capturable.
 */
#ifndef SELFTOK_HIP_EXT_H
#define SELFTOK_HIP_EXT_H

#include "selftok_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- two-segment attention with a per-sample key bit mask ---------------------------------------
 * selftok_attn_f32 with ANY visibility pattern over the seg[0] keys instead of the prefix j <= kvis[b]: the reference's
 * materialised mask (sd3/mmdit.py:1059-1094) for `mask * super_mask` with a [B, K] super_mask (rectified_flow.py:226-227).
 * Bit (j & 31) of word kmask[b * kmask_bs + (j >> 5)] is 1 iff seg[0] key j of sample b is visible (to every row);
 * bits at j >= seg[0].len are ignored.  A seg[0] ROW whose bit is clear is dead and is not written.  The output does not
 * depend on the contents of an invisible key (NaN and Inf included), and such a key cannot raise the f16x2 overflow flag.
 * 32-key tiles without a visible key are skipped; 128-row query tiles without a live row return at once.
 * desc->kvis must be NULL, head_dim 64 only, seg[0].len <= 2048, kmask_bs >= ceil(seg[0].len / 32); everything else
 * (seg[1], seg0_sees_seg1, strides, mode, overflow, o_blk) means what it means in selftok_attn_f32. */
int selftok_attn_kmask_f32(const selftok_attn_desc* desc, const unsigned* kmask, long kmask_bs, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SELFTOK_HIP_EXT_H */
