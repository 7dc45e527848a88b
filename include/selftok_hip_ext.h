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

/* ---- exact-order attention with a per-sample key bit mask ----------------------------------------
 * The two exact-order attention entries of selftok_hip.h (ATen's fp32 CPU flash kernel, bit for bit; unfused and fused) with ANY
 * visibility pattern over the first segment's Tk1 key slots: the boolean mask the reference hands to SDPA is the same ATen code
 * path for a prefix and for every other pattern.  The bit layout is selftok_attn_kmask_f32's: slot j of sample b is visible iff
 * j < valid1 and bit (j & 31) of word kmask[b * kmask_bs + (j >> 5)] is set (`mask * super_mask`: the step prefix and the pattern
 * combine); kmask_bs == 0: one pattern for the whole batch, else kmask_bs >= ceil(Tk1 / 32).  Tk1 <= 2048.  The second segment is
 * always visible.  A masked key keeps its slot in the 512-key blocks, adds an exact zero and is never read into the arithmetic
 * (NaN and Inf included): prefix bits give the bits of the entries without a mask.  A sample without any visible key is legal
 * here: the fused entry does not write its rows, the unfused one writes zeros -- pass a zero-filled `out` when that can happen
 * (ATen yields NaN there).  Every other argument and constraint is that of the entry without a mask. */
int selftok_ex_attention_kmask_f32(const float* q, long qs, const float* k1, const float* v1, long kvs1, int Tk1, int valid1, int rows1, const float* k2, const float* v2,
                                   long kvs2, int Tk2, float* out, void* workspace, int B, int H, int Tq, int D, const unsigned* kmask, long kmask_bs, hipStream_t stream);
int selftok_ex_attention_kmask_fused_f32(const float* q, long qs, const float* k1, const float* v1, long kvs1, int Tk1, int valid1, int rows1, const float* k2, const float* v2,
                                         long kvs2, int Tk2, float* out, int B, int H, int Tq, int D, const unsigned* kmask, long kmask_bs, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SELFTOK_HIP_EXT_H */
