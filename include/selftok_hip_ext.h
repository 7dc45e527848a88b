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

/* ---- device image input: PIL-exact Resize(S) -> CenterCrop(S) -> NormalizeToTensor -------------------
 * B RGB uint8 HWC images of different sizes, packed into one device buffer, -> out [B, 3, S, S] in [-1, 1].  `table` holds three longs
 * per image: byte offset into `packed`, width, height; it is passed twice, readable by the host (validation, launch sizes) and by the
 * device (the kernels) -- the same values, the caller's copy.  The device re-checks every image of ITS copy against the limits the host
 * copy sized the launch and the workspace for: an image whose device entry disagrees is not processed -- its output planes are left
 * untouched and the call still returns 0 (nothing is read or written outside; keeping the copies equal is the caller's duty).
 * Per image, bit for bit what the reference's user script computes:
 *   shorter side -> S, the other (int)(S * long / short); Pillow's 8-bit bilinear resample with antialias (ImagingResample: horizontal
 *   pass first, uint8 between the passes, fp64 weights, 22-bit fixed-point coefficients, (2^21 + sum) >> 22, clip); a side that already
 *   has its length is not resampled; centre crop at int(round((side - S) / 2.0)), half to even; then lut[u8].
 * Only the crop window is resampled.  `lut`: 256 device values of the output type, float32(u8) / 127.5 - 1.0 made by the caller with the
 * host expression it must equal (fp32, or that rounded to bf16).  out_bf16 != 0: out and lut are bf16, else fp32.
 * Limits: 1 <= S <= 4096, 1 <= side <= 65536, a resized side < 2^30, offset + 3 * w * h <= packed_bytes.  The workspace (coefficient tables
 * and the uint8 rows between the passes) is sized by the query from the same host table; 0 with selftok_last_error set on a bad table.
 * After the call the workspace holds, per image b and output index i of the crop window, the tap rows
 *   ((int*)workspace)[hdr + (b * S + i) * ks + {0: first input index, 1: taps n, 2 .. 2 + n: coefficients}]
 * with hdr / ks / the vertical tables' base from selftok_img_resize_tables_layout (ints: [0] base of the horizontal tables,
 * [1] their row stride, [2] base of the vertical tables, [3] their row stride; all in ints from the workspace start). */
size_t selftok_img_resize_crop_norm_u8_workspace_bytes(const long* table_host, int B, int S);
int selftok_img_resize_tables_layout(const long* table_host, int B, int S, long* layout4);
int selftok_img_resize_crop_norm_u8(const unsigned char* packed, size_t packed_bytes, const long* table_host, const long* table_dev, int B, int S, void* out,
                                    int out_bf16, const void* lut, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* ---- device image views: crop box -> resize -> S x S window -> flip -> NormalizeToTensor, PIL-exact ----
 * V outputs [V, 3, S, S] taken from RGB uint8 HWC sources packed into one device buffer; several views may name the same source, which
 * lies in `packed` once.  One row of twelve longs per OUTPUT: byte offset of the source, its width W and height H; the crop box x0, y0,
 * bw, bh; the size Rw, Rh the box is resized to; the window's left, top inside Rw x Rh; flip (0 or 1).  Per view, bit for bit:
 *   im = source.crop((x0, y0, x0 + bw, y0 + bh)); im = im.resize((Rw, Rh), BILINEAR) unless (Rw, Rh) == (bw, bh);
 *   im = im.crop((left, top, left + S, top + S)); im = im.transpose(FLIP_LEFT_RIGHT) if flip; out = lut[im]
 * with the resample of selftok_img_resize_crop_norm_u8 (horizontal pass first, uint8 between the passes, fp64 weights, 22-bit
 * coefficients, (2^21 + sum) >> 22, clip; an axis whose length does not change is not resampled).  Crop-then-resize, as torchvision's
 * resized_crop does it: NOT Pillow's resize(box=), whose taps reach outside the box.  Only the window is resampled; the flip is a
 * reversed column index at the store.  torchvision's FiveCrop / TenCrop / RandomResizedCrop / hflip are choices of these numbers.
 * The table is passed twice like the table of selftok_img_resize_crop_norm_u8 and under the same rule: the host copy is validated
 * (SELFTOK_EINVAL with a message, nothing launched), the device re-checks ITS copy against the limits and the sizes the host copy gave
 * the launch, and a view that disagrees is skipped: its output planes stay untouched, nothing is read or written outside, return 0.
 * Limits: 1 <= V <= 65535, 1 <= S <= 4096, 1 <= W, H <= 65536, the box inside the source with bw, bh >= 1, S <= Rw, Rh < 2^30, the window
 * inside Rw x Rh, offset + 3 * W * H <= packed_bytes.  `lut`, out_bf16, the workspace query and the tap rows left in the workspace
 * (per view v and window index i, at hdr + (v * S + i) * ks, box coordinates) are those of the entry above, with
 * selftok_img_views_tables_layout giving hdr / ks. */
size_t selftok_img_views_u8_workspace_bytes(const long* views_host, int V, int S);
int selftok_img_views_tables_layout(const long* views_host, int V, int S, long* layout4);
int selftok_img_views_u8(const unsigned char* packed, size_t packed_bytes, const long* views_host, const long* views_dev, int V, int S, void* out, int out_bf16,
                         const void* lut, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* ---- device image views with a chosen Pillow filter ------------------------------------------------------
 * selftok_img_views_u8 with one more argument, `filter`, Pillow's own code: BILINEAR = 2, BICUBIC = 3 (a = -0.5, support 2), BOX = 4
 * (1 on -0.5 < x <= 0.5, support 0.5).  The same [V, 12] rows, limits, host-table / device-table rule, lut, outputs and workspace layout;
 * the tap rows are as wide as the filter needs, ksize = 2 * ceil(support * max(scale, 1)) + 1, and the query and the layout call take
 * the filter too.  filter = 2 gives the bits and the tap rows of selftok_img_views_u8.  LANCZOS (1) and HAMMING (5) are refused by name:
 * their weights are libm's sin / cos, whose bits the device does not promise; NEAREST (0) is refused too (Pillow does not resample it
 * through coefficient tables).  SELFTOK_EINVAL, nothing launched. */
size_t selftok_img_views_filter_u8_workspace_bytes(const long* views_host, int V, int S, int filter);
int selftok_img_views_filter_tables_layout(const long* views_host, int V, int S, int filter, long* layout4);
int selftok_img_views_filter_u8(const unsigned char* packed, size_t packed_bytes, const long* views_host, const long* views_dev, int V, int S, int filter, void* out,
                                int out_bf16, const void* lut, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* ---- device whole-frame resize: Pillow's Image.resize((ow, oh), filter) on uint8 HWC frames ---------------
 * N frames that lie in `packed` are resized into other regions of the SAME buffer (the BOX halvings of the ADM centre crop are chains of
 * such calls).  One row of six longs per frame: source byte offset, W, H, destination byte offset, ow, oh; the table is passed twice,
 * under the rule of the entries above.  Per frame, bit for bit: horizontal pass first, uint8 between the passes, an axis whose length does
 * not change is not resampled, fp64 weights, 22-bit coefficients, (2^21 + sum) >> 22, clip.  `filter` as above.
 * The host copy is validated (SELFTOK_EINVAL with a message, nothing launched): 1 <= N <= 65535, 1 <= W, H, ow, oh <= 65536, every
 * source and destination region inside packed_bytes, no destination region overlapping any source or destination region of the call
 * (sources may coincide).  The device re-checks ITS copy against the same rules and against what the host copy sized the launch and the
 * workspace for; a frame that disagrees is skipped, its destination stays untouched, return 0.  The workspace (tap rows of every frame
 * and its H x ow uint8 rows between the passes) is sized by the query, 0 with selftok_last_error set on a bad table; 16-byte aligned. */
size_t selftok_img_resize_u8_workspace_bytes(const long* frames_host, int N, int filter);
int selftok_img_resize_u8(unsigned char* packed, size_t packed_bytes, const long* frames_host, const long* frames_dev, int N, int filter, void* workspace,
                          size_t workspace_bytes, hipStream_t stream);

/* ---- device image output: [B, 3, H, W] in [0, 1] -> uint8 [B, H, W, 3] ---------------------------------
 * torchvision.utils.save_image's arithmetic in the tensor's own type: x * 255 rounded to the type, + 0.5 rounded to the type, clamp to
 * [0, 255], truncate.  in_bf16 != 0: bf16 input, else fp32.  +Inf -> 255, -Inf -> 0; NaN -> 0 (this project's choice: torch's
 * float -> uint8 conversion of NaN is undefined).  B * H * W < 2^31. */
int selftok_img_to_u8(const void* img, int in_bf16, unsigned char* out, int B, int H, int W, hipStream_t stream);

/* ---- device image metrics: per-image SSIM and mean squared error in one pass ----------------------------
 * recon [B, 3, H, W] in [0, 1] (recon_bf16 != 0: bf16, else fp32) against orig [B, 3, H, W] (orig_bf16 likewise), both contiguous ->
 * out [B][2] fp64 on the device: {mean SSIM, MSE} of each image.  orig_signed != 0: the original is in [-1, 1] and becomes
 * o = (float32(v) + 1) / 2 in fp32 (evaluate.psnr_each's expression), else o = float32(v).
 * SSIM: Wang et al., the 11 x 11 separable window whose 11 fp64 weights the caller passes in `window11_host` (host memory, copied into
 * the launch; normally the normalised Gaussian of sigma 1.5), "valid" windows only ((H - 10) x (W - 10) of them per channel, no padding),
 * population moments, C1 = 0.01^2, C2 = 0.03^2 (data range 1), every operation in fp64 and rounded on its own, the fp64 mean over the three
 * channels and all windows.  MSE: d = float32(recon) - o and d * d in fp32, summed in fp64, divided by 3 * H * W; PSNR is the caller's
 * 10 * log10(1 / MSE).  quantize != 0: both inputs first become the bytes of selftok_img_to_u8 (the reconstruction in its own type, o in
 * fp32), SSIM is taken on byte / 255.0 in fp64 and MSE is the exact integer sum of (bx - by)^2 divided by 65025 * 3 * H * W.
 * No atomics: out[b] is a function of image b alone, bit-identical from run to run and for any batch around it.
 * Limits: B >= 1, H, W >= 11, B * 3 * H * W < 2^31.  The workspace (one pair of partial sums per tile) is sized by the query; 0 with
 * selftok_last_error set on a refused shape. */
size_t selftok_img_metrics_workspace_bytes(int B, int H, int W);
int selftok_img_metrics(const void* recon, int recon_bf16, const void* orig, int orig_bf16, int orig_signed, int quantize, const double* window11_host, double* out,
                        void* workspace, size_t workspace_bytes, int B, int H, int W, hipStream_t stream);

/* ---- VQ lookup: the k best codes of every row with their exact scores ------------------------------------
 * z [N, 16] fp32 and `packed` (selftok_vq_pack_codebook) as for selftok_vq_encode_packed_f32 -> ids [N, k] (int64, or int32 with
 * SELFTOK_IDS_I32) and scores [N, k] fp32.  With x = l2norm16(z[n]) (SELFTOK_PRENORMED: x = z[n]) and s[c] the canonical k-ordered fp32
 * FMA chain of the argmax entries, row n receives the first k codes in this order -- defined here, NOT torch.topk's, which promises none
 * among ties:
 *   score descending; equal scores (-0.0 == +0.0) by ascending code index; NaN scores before every number, among themselves by
 *   ascending index.  A zero score is written as +0.0 and a NaN score as the quiet NaN 0x7FC00000, as `best` is.
 * Column 0 is bit for bit the (ids, best) of selftok_vq_encode_packed_f32.  The [N, C] score matrix is never materialised.
 * flags: SELFTOK_IDS_I32, SELFTOK_PRENORMED, and the launch-shape overrides SELFTOK_VQ_RT(1|2|4) / SELFTOK_VQ_SPLIT(n), on which the
 * outputs never depend (a split count above min(64, C / 32) is ignored).  1 <= k <= 8, D == 16, C % 32 == 0: anything else returns
 * SELFTOK_EINVAL with a message in selftok_last_error and launches nothing.  N == 0 returns 0 and writes nothing.
 * Workspace: min(64, C / 32) * max(N, 1) * kpad * 8 bytes, kpad = k rounded up to 1, 2, 4 or 8 -- one sorted list of kpad 64-bit keys
 * (orderable(score) << 32 | 0xFFFFFFFF - code) per code split and row; it does not grow with N * C.  The query returns 0 with
 * selftok_last_error set for k, C or N out of range. */
size_t selftok_vq_topk_workspace_bytes(int N, int C, int k);
int selftok_vq_topk_packed_f32(const float* z, const float* packed, void* ids, float* scores, void* workspace,
                               int N, int C, int D, int k, int flags, hipStream_t stream);

/* ---- single-pass fp16 Linear on the split planes (the "f16" GEMM mode) ---------------------------------
 * The two pre-split f16x2 Linears of selftok_hip.h (selftok_linear_f16x2_split, selftok_linear_f16x2_split_residual) with both
 * LOW planes taken as zero:
 *     out = act(fp16(A) fp16(W)^T + bias),  fp16-rounded operands, fp32 accumulation, one matrix instruction per product
 * -- a LOSSY mode (11 significand bits per operand), not fp32-equivalent.  Same argument lists, same inputs: `a_blk` is a split
 * activation [M, K] and `packed` the image of selftok_linear_f16x2_pack_weight; only their hi planes are read (the lo planes may
 * hold anything).  Every output is the ascending-k chain of 16-deep steps of the f16x2 kernel's high accumulator and the epilogue
 * is that kernel's with lo = 0, so on operands that are exactly representable in fp16 the results equal the f16x2 entries'.
 * flags: SELFTOK_LINEAR_GELU.  Output: fp32 `out` (row stride ldo, out_blk = NULL) or a split activation [M, N] with BOTH planes
 * (out = NULL).  The residual entry computes resid + gate * (A W^T + bias) as selftok_linear_f16x2_split_residual does (gate NULL,
 * per-sample or per-token table).  overflow bit 0 is OR-ed for a non-finite output (an |activation| >= 65504 is one).
 * Refusals as the f16x2 entries: N % 128, K % 32, null / unaligned pointers, bad strides -> SELFTOK_EINVAL; M == 0 returns 0 without
 * a launch.  These two entries walk all of K in one work-group per output tile; small row counts (one to four images) belong on
 * selftok_linear_f16x2_split_k, or -- staying in this lossy arithmetic -- on the split-K variants below. */
int selftok_linear_f16_split(const void* a_blk, const void* packed, const float* bias, float* out, void* out_blk, long ldo,
                             int M, int N, int K, int flags, int* overflow, hipStream_t stream);
int selftok_linear_f16_split_residual(const void* a_blk, const void* packed, const float* bias,
                                      const float* resid, long ldr, const float* gate, long gate_stride_b, long gate_stride_t, int T,
                                      float* out, long ldo, int M, int N, int K, int* overflow, hipStream_t stream);

/* Split-K variants of the two entries above (csrc/gemm_f16_splitk.hip), with the argument lists of selftok_linear_f16x2_split_k /
 * selftok_linear_f16x2_split_residual_k: `ksplit` work-groups share an output tile, each over K / 32 / ksplit consecutive k-tiles in
 * ascending 16-deep steps, and write raw fp32 partial sums to plane s of `workspace` ([ksplit][M][N] fp32, 16-byte aligned,
 * its size in bytes is what selftok_linear_f16x2_splitk_workspace_bytes returns; nothing beyond is touched); the second launch is the f16x2 route's
 * reduction: planes added in ascending order, then bias and the epilogue.  Deterministic.  LOSSY as above; on operands exactly
 * representable in fp16 the results equal those of the f16x2 _k entries with the same ksplit, bit for bit.  ksplit == 1 forwards to
 * the single-pass entry (workspace not read).  Refused (SELFTOK_EINVAL) on top of the refusals above, exactly as the f16x2 _k entries
 * refuse: ksplit < 1 or > 64, ksplit not a divisor of K / 32, workspace NULL or not 16-byte aligned. */
int selftok_linear_f16_split_k(const void* a_blk, const void* packed, const float* bias, float* out, void* out_blk, long ldo,
                               int M, int N, int K, int flags, int ksplit, void* workspace, int* overflow, hipStream_t stream);
int selftok_linear_f16_split_residual_k(const void* a_blk, const void* packed, const float* bias,
                                        const float* resid, long ldr, const float* gate, long gate_stride_b, long gate_stride_t, int T,
                                        float* out, long ldo, int M, int N, int K, int ksplit, void* workspace, int* overflow, hipStream_t stream);

/* ---- single-pass fp16 joint attention (the attention of the "f16" mode) ---------------------------------
 * selftok_attn_f32 / selftok_attn_kmask_f32 with ONE fp16 matrix instruction per product -- LOSSY (11 significand bits per
 * operand), not fp32-equivalent.  Arithmetic of record, operands fp32 q, k, v, head_dim 64:
 *     c = scale * 1.4426950408889634f (fp32 product);  q~ = fp16(q * c) (fp32 multiply, then round to nearest even);
 *     k~ = fp16(k), v~ = fp16(v);  s_j = sum_d q~_d k~_jd (exact fp16 products, fp32 accumulation, log2 domain);
 *     online softmax in fp32 against the true running maximum;  p~ = fp16(exp2(s - m));  O += v~^T p~;  the row sum adds the
 *     rounded p~ in fp32;  o = O / l -- a convex combination of fp16(v) rows up to fp32 rounding.
 * The descriptor is selftok_attn_f32's.  kmask == NULL: desc->kvis rules (may be NULL).  Otherwise the words and limits of
 * selftok_attn_kmask_f32: kvis must be NULL, seg[0].len <= 2048, kmask_bs >= ceil(seg[0].len / 32).  Visibility, dead rows
 * (not written) and seg0_sees_seg1 are those entries'; an invisible key contributes an exact zero and its contents (NaN and Inf
 * included) reach neither the output nor the flag.  desc->mode is not read.  Output per segment: fp32 `o`, or a split activation
 * desc->o_blk[s] (16-byte aligned) with BOTH planes, the lo plane being the residual of the fp32 output.  |q * c|, |k| or
 * |v| >= 65504 gives a non-finite output and ORs bit 2 into *desc->overflow.  head_dim != 64 returns SELFTOK_EINVAL with a
 * message; B == 0 or no query row returns 0 without a launch. */
int selftok_attn_f16(const selftok_attn_desc* desc, const unsigned* kmask, long kmask_bs, hipStream_t stream);

/* ---- LPIPS stages (AlexNet backbone): fp32 convolution, max-pool, input stage, fp64 distance stage ------------
 * The kernels of selftoktokenizer_amd/lpips.py (LPIPS_DEFINITION states the metric; csrc/lpips.hip states the arithmetic).  Activations
 * are channels-last fp32 [N, H, W, C], contiguous.  Every refusal (null pointer, a shape without an output pixel, an element count
 * >= 2^31, a short workspace) is decided on the host before any launch and returns SELFTOK_EINVAL with a message.
 *
 * selftok_lpips_conv2d_f32: cross-correlation with zero padding, + bias (NULL: none), + ReLU when relu != 0, in [N, H, W, Cin] ->
 *   out [N, OH, OW, Cout], OH = (H + 2 pad - KH) / stride + 1 (floor).  `packed` is the weight [Cout, Cin, KH, KW] re-laid as
 *   [KP][CoutP] fp32 with row k = (kh * KW + kw) * Cin + ci, KP = K rounded up to 16, CoutP = Cout rounded up to 64, the padding
 *   zero-filled; selftok_lpips_conv2d_packed_floats returns KP * CoutP (0 with the error set when refused).  fp32 operands and
 *   accumulation on v_mfma_f32_32x32x2_f32: every output is eight fmaf chains from +0.0f (chain j: the taps with k mod 16 in {2j, 2j + 1},
 *   ascending; a padding tap is an exact zero, never a neighbour's value) added as a fixed fp32 tree, then one fp32 addition of the bias,
 *   then v < 0 ? 0 : v.  An output depends on its own image alone.
 *   0 <= pad < KH, KW;  `in` and `packed` 16-byte aligned.
 * selftok_lpips_maxpool3s2_f32: 3 x 3 windows, stride 2, no padding, floor mode: [N, H, W, C] -> [N, (H - 3) / 2 + 1, (W - 3) / 2 + 1, C];
 *   a NaN in a window is the window's result.  H, W >= 3.
 * selftok_lpips_input: recon [B, 3, H, W] in [0, 1] and orig [B, 3, H, W] (bf16 or fp32 each, NCHW) -> out [2B, H, W, 3], recon images
 *   first: x = float32(v) * 2 - 1 (two fp32 roundings; a signed original is taken as it is), or with quantize != 0
 *   x = byte / 255 * 2 - 1 in fp32 of the byte selftok_img_metrics takes (recon in its own type; the original from
 *   o = (v + 1) / 2 when signed, as fp32), then the scaling layer (x - shift_c) / scale_c in fp32 with a true division,
 *   shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450).  H, W >= 31: below that a tap of the network has no pixel.
 * selftok_lpips_distance: feat [2B, npix, C] (images b and b + B are pair b) and w [C] -> out[b] (fp64, device) = the tap's contribution
 *   mean_p sum_c w_c (f0_c / n0 - f1_c / n1)^2, n = sqrt(sum_c f_c^2) + 1e-10, every operation in fp64 and rounded on its own, sums in a
 *   fixed order (csrc/lpips.hip), no atomics: out[b] is a function of pair b alone.  accumulate != 0: out[b] += instead of =.
 *   Workspace (one fp64 per 64-pixel tile and pair) from the query; 0 with the error set when B or npix is refused.  B <= 65535. */
size_t selftok_lpips_conv2d_packed_floats(int Cin, int Cout, int KH, int KW);
int selftok_lpips_conv2d_f32(const float* in, const float* packed, const float* bias, float* out, int N, int H, int W, int Cin, int Cout,
                             int KH, int KW, int stride, int pad, int relu, hipStream_t stream);
int selftok_lpips_maxpool3s2_f32(const float* in, float* out, int N, int H, int W, int C, hipStream_t stream);
int selftok_lpips_input(const void* recon, int recon_bf16, const void* orig, int orig_bf16, int orig_signed, int quantize, float* out,
                        int B, int H, int W, hipStream_t stream);
size_t selftok_lpips_distance_workspace_bytes(int B, int npix);
int selftok_lpips_distance(const float* feat, const float* w, double* out, void* workspace, size_t workspace_bytes, int B, int npix, int C,
                           int accumulate, hipStream_t stream);

/* ---- LPIPS on the VGG16 backbone: the 2 x 2 max-pool (csrc/lpips_vgg.hip) -----------------------------------------
 * lpips.py's LPIPS_VGG_DEFINITION states the metric.  The 13 convolutions (3 x 3, pad 1, stride 1, ReLU) run on selftok_lpips_conv2d_f32
 * and the input and distance stages are the ones above; the only stage VGG16 adds is torchvision's MaxPool2d with kernel 2 and stride 2:
 * 2 x 2 windows, stride 2, no padding, floor mode: [N, H, W, C] -> [N, H / 2, W / 2, C], the last row / column of an odd map is dropped;
 * a NaN in a window is the window's result.  H, W >= 2, N * H * W * C < 2^31; refusals are decided on the host before any launch. */
int selftok_lpips_maxpool2s2_f32(const float* in, float* out, int N, int H, int W, int C, hipStream_t stream);

/* ---- SSIM with a caller-chosen window and moment convention (csrc/image_ssim.hip) ------------------------------------
 * recon [B, 3, H, W] in [0, 1] and orig [B, 3, H, W] as selftok_img_metrics takes them (bf16 or fp32 each; orig_signed != 0: the original is
 * in [-1, 1]) -> out[B] fp64 on the device: the mean SSIM of each image over the three channels and the (H - taps + 1) x (W - taps + 1)
 * "valid" windows -- what scikit-image's crop by (taps - 1) / 2 of its reflect-padded map leaves.
 * window_host: `taps` separable fp64 weights in host memory (copied into the launch), taps odd, 3 <= taps <= 11.
 * cov_norm: 1.0 for population moments, taps^2 / (taps^2 - 1) for scikit-image's use_sample_covariance=True.
 * signed_range == 0: operands on [0, 1], C1 = 0.01^2, C2 = 0.03^2, selftok_img_metrics' own operand expressions;
 * signed_range != 0: operands on [-1, 1], data range R = 2, C1 = (0.01 R)^2, C2 = (0.03 R)^2: the reconstruction is 2 r - 1 in fp64, a signed
 *   original is taken as it is, an unsigned one is 2 v - 1.  quantize != 0: both inputs first become the bytes of selftok_img_to_u8 (as in
 *   selftok_img_metrics), the operand is byte / 255 or 2 * (byte / 255) - 1 in fp64.
 * Arithmetic, fp64 and every operation rounded on its own: the five window filters (horizontal pass, then vertical, taps ascending) ux, uy,
 *   uxx, uyy, uxy; vx = cov_norm * (uxx - ux * ux), vy likewise, vxy = cov_norm * (uxy - ux * uy);
 *   S = ((2 ux uy + C1) * (2 vxy + C2)) / ((ux^2 + uy^2 + C1) * (vx + vy + C2)).  This is the fp64 form: scikit-image >= 0.19 computes float32
 *   input in float32, which is not imitated; unpinned against the package.
 * With the 11 Gaussian weights, cov_norm 1.0 and signed_range 0 the result is column 0 of selftok_img_metrics bit for bit (the same
 * operations in the same order).  No atomics: out[b] is a function of image b alone; identical images give exactly 1.0.
 * Limits: B >= 1, H, W >= taps, B * 3 * H * W < 2^31, 0 < cov_norm <= 2.  The workspace (one fp64 per tile) is sized by the query; 0 with
 * selftok_last_error set on a refused shape or window.  Every refusal is decided on the host before any launch. */
size_t selftok_img_ssim_workspace_bytes(int B, int H, int W, int taps);
int selftok_img_ssim(const void* recon, int recon_bf16, const void* orig, int orig_bf16, int orig_signed, int quantize, const double* window_host, int taps,
                     double cov_norm, int signed_range, double* out, void* workspace, size_t workspace_bytes, int B, int H, int W, hipStream_t stream);

/* ---- rFID stages (FID InceptionV3, pool3): convolution into a channel slice, 3 x 3 pools, input stage with resize, spatial mean,
 *      fp64 statistics ----------------------------------------------------------------------------------------------
 * The kernels of selftoktokenizer_amd/fid.py (FID_DEFINITION states the metric; csrc/fid.hip states the arithmetic and every summation
 * order).  Activations are channels-last fp32.  An output MAP has rows of `ldo` floats; an entry writes the channels co_off ..
 * co_off + C - 1 of every output pixel and leaves every other byte of the map alone (0 <= co_off, co_off + C <= ldo), so the branches
 * of an Inception block write one concatenated map.  Every refusal is decided on the host before any launch and returns SELFTOK_EINVAL
 * with a message; an output depends on its own image alone.
 *
 * selftok_fid_conv2d_f32: selftok_lpips_conv2d_f32 (the same kernel body, arithmetic and packed weight: selftok_lpips_conv2d_packed_floats)
 *   with a padding per axis, 0 <= pad_h < KH and 0 <= pad_w < KW, and the slice.  ldo = Cout, co_off = 0, pad_h = pad_w gives the LPIPS
 *   entry's bits.
 * selftok_fid_pool3_f32: 3 x 3 windows.  mode 0: max, stride 2, no padding (floor; H, W >= 3); mode 1: max, stride 1, pad 1 (a padding
 *   tap never takes part); mode 2: average, stride 1, pad 1, divisor = the number of in-image taps (count_include_pad=False): the taps
 *   added from +0.0f in (kh, kw) order in fp32, then one division.  A NaN in a window is the window's result.
 * selftok_fid_input: src [B, 3, H, W] (bf16 or fp32, NCHW) -> out [B, OH, OW, 3] in [-1, 1]: x = float32(v) * 2 - 1 of a [0, 1] image
 *   (src_signed == 0), a signed image as it is; quantize != 0: byte / 255 * 2 - 1 of the byte selftok_lpips_input takes (an unsigned
 *   image in its own type, a signed one from (v + 1) / 2 in fp32).  ytab / xtab (device, both or neither): 3 * OH (3 * OW) ints, i0[],
 *   i1[] and the bits of the fp32 lambda[] of every output row (column); the converted values are blended in fp32, each operation rounded
 *   on its own, top = a + lx * (b - a), bot = c + lx * (d - c), x = top + ly * (bot - top).  Indices are clamped into the image.
 *   Without tables OH x OW must be H x W and the converted values are stored as they are.
 * selftok_fid_spatial_mean_f32: in [N, npix, C] -> out [N, C]: the pixels added from +0.0f in index order in fp32, then / (float)npix.
 * selftok_fid_stats: x [N, D] fp32 -> mu [D] and sigma [D, D] fp64 (device), sigma the unbiased covariance (1 / (N - 1)), two passes
 *   in fp64 in the fixed order csrc/fid.hip states (chunks of 256 rows ascending, a fixed pairwise tree across chunks), no atomics;
 *   sigma is exactly symmetric.  2 <= N <= 256 * 65535, D % 16 == 0.  Workspace (one fp64 per chunk and column) from the query; 0 with
 *   the error set when N or D is refused. */
int selftok_fid_conv2d_f32(const float* in, const float* packed, const float* bias, float* out, int N, int H, int W, int Cin, int Cout,
                           int KH, int KW, int stride, int pad_h, int pad_w, int ldo, int co_off, int relu, hipStream_t stream);
int selftok_fid_pool3_f32(const float* in, float* out, int N, int H, int W, int C, int mode, int ldo, int co_off, hipStream_t stream);
int selftok_fid_input(const void* src, int src_bf16, int src_signed, int quantize, float* out, int B, int H, int W, int OH, int OW,
                      const int* ytab, const int* xtab, hipStream_t stream);
int selftok_fid_spatial_mean_f32(const float* in, float* out, int N, int npix, int C, hipStream_t stream);
size_t selftok_fid_stats_workspace_bytes(int N, int D);
int selftok_fid_stats(const float* x, double* mu, double* sigma, void* workspace, size_t workspace_bytes, int N, int D, hipStream_t stream);

/* ---- generative-model metrics: k-NN radii and manifold membership on squared distances, Inception Score reductions ------------
 * The kernels of selftoktokenizer_amd/genmetrics.py (GEN_METRICS_DEFINITION states the metrics; csrc/gen_metrics_shared.h states the
 * arithmetic of d2(u, v) = |u|^2 + |v|^2 - 2 u.v clamped at +0, SQUARED and never square-rooted, its bits a function of the two rows
 * alone; csrc/gen_metrics.hip states the selection and every summation order).  Rows are contiguous fp32 [., D], D a multiple of 16 in
 * 16 .. 2048, 16-byte aligned.  The N x N / M x N distance matrix is never stored.  Every refusal is decided on the host before any
 * launch and returns SELFTOK_EINVAL with a message (the queries return 0 with the message set); nothing allocates, synchronises or
 * keeps state; no atomics.
 *
 * selftok_knn_radius_f32: a [N, D] -> r2[j] = the k-th smallest d2(a_j, a_i) over i != j (the row's own INDEX is skipped, not its value:
 *   a bit-copy of row j is a neighbour, at a distance within E of 0 -- the same bits through both entries).  1 <= k <= 8, N > k.  A NaN distance is never a neighbour; a row with fewer
 *   than k non-NaN neighbours (a row that holds a NaN) gets r2 = NaN and changes no other row's radius.
 * selftok_manifold_member_f32: x [M, D], a [N, D], r2 [N] -> member[i] = 1 if d2(x_i, a_j) <= r2[j] for some j, else 0 (int32).  The
 *   comparison is <=, false against NaN.  M == 0 returns 0 without a launch.
 * `split`: launch-shape override, the number of column splits (0 = automatic; values above min(64, ceil(N / 128)) are clamped); the
 *   outputs never depend on it.  Workspace (row norms, and per column part and row the k smallest distances / one flag) from the
 *   queries; nothing beyond the stated size is touched.
 * selftok_is_colmean: logits [N, C] fp32 -> colmean [ceil(N / split_size), C] fp64: per consecutive split of split_size rows (the last,
 *   partial split included) the column means of p = softmax(logits) taken in fp64, chunks of 256 rows and a fixed pairwise tree.
 * selftok_is_kl_rows: kl[n] = sum_y p_ny (log p_ny - log colmean[n / split_size][y]) in fp64; a term with p_ny == 0 is 0.
 *   N, C, split_size >= 1, N * C < 2^31, at most 65535 chunks over all splits. */
size_t selftok_knn_radius_f32_workspace_bytes(int N, int D, int k);
int selftok_knn_radius_f32(const float* a, float* r2, void* workspace, size_t workspace_bytes, int N, int D, int k, int split, hipStream_t stream);
size_t selftok_manifold_member_f32_workspace_bytes(int M, int N, int D);
int selftok_manifold_member_f32(const float* x, const float* a, const float* r2, int* member, void* workspace, size_t workspace_bytes, int M, int N, int D,
                                int split, hipStream_t stream);
size_t selftok_is_colmean_workspace_bytes(int N, int C, int split_size);
int selftok_is_colmean(const float* logits, double* colmean, void* workspace, size_t workspace_bytes, int N, int C, int split_size, hipStream_t stream);
size_t selftok_is_kl_rows_workspace_bytes(int N, int C, int split_size);
int selftok_is_kl_rows(const float* logits, const double* colmean, double* kl, void* workspace, size_t workspace_bytes, int N, int C, int split_size,
                       hipStream_t stream);

/* ---- density / coverage, nearest neighbours and KID on the same features (csrc/gen_metrics_kdc.hip) --------------------------------
 * The pair arithmetic is csrc/gen_metrics_shared.h's: d2 and the dot products carry the bits the two entries above produce.  Limits,
 * alignment, refusals and the `split` override are theirs too.  Unpinned against torch-fidelity and prdc.
 *
 * manifold_count_nn: x [M, D], a [N, D], r2 [N] or null -> count[i] = #{ j : d2(x_i, a_j) <= r2[j] } (int32; <= as the membership entry,
 *   false against NaN; count is null exactly when r2 is, and then no count is taken), nn_d2[i] = the smallest non-NaN d2(x_i, a_j),
 *   nn_idx[i] = the lowest j whose d2 has those bits (the minimum of (bits of d2 << 32) | j as an unsigned 64-bit integer); a query with
 *   no non-NaN distance gets nn_d2 = NaN, nn_idx = -1.  Rows past the end of the set are masked by index.  M == 0 returns 0 without a
 *   launch.  Workspace: the row norms, and per column part and query one 64-bit key and one count.
 * kid_sums: xs, ys [S * m, D]: subset s is rows s * m .. s * m + m - 1 of either -> sums [S, 3] fp64 = { XX, YY, XY } with
 *   k(u, v) = (u.v / D + 1)^3: the dot product c is the shared fp32 chain, t = (double)c / (double)D + 1.0 and (t * t) * t are fp64;
 *   XX = sum over positions i != j of k(x_i, x_j) (the diagonal excluded by position, not by value), YY likewise, XY = sum over all i, j.
 *   The summation order is fixed (csrc/gen_metrics_kdc.hip states it); a subset's triple depends on its own 2 m rows alone.
 *   1 <= S <= 65535, 2 <= m <= 2^22, S * m * D < 2^31.  Workspace: one fp64 per (subset, sum, 128 x 128 tile). */
size_t selftok_manifold_count_nn_f32_workspace_bytes(int M, int N, int D);
int selftok_manifold_count_nn_f32(const float* x, const float* a, const float* r2, int* count, float* nn_d2, int* nn_idx, void* workspace, size_t workspace_bytes,
                                  int M, int N, int D, int split, hipStream_t stream);
size_t selftok_kid_sums_f32_workspace_bytes(int S, int m, int D);
int selftok_kid_sums_f32(const float* xs, const float* ys, double* sums, void* workspace, size_t workspace_bytes, int S, int m, int D, hipStream_t stream);

/* ---- decode stream: one sampler step per slot (csrc/decode_stream.hip) --------------------------------------------------------------
 * A batch of B slots in which slot b is at its own sampler step step[b] (int32, device).  A slot is ACTIVE iff 0 <= step[b] < n_steps.
 * Both entries are stateless, capturable, without workspace, atomics or scratch; every refusal is decided on the host (SELFTOK_EINVAL with
 * a message, nothing launched).
 *
 * stream_prepare: limit [n_steps] int32 = min(k + 1, K) of every step; coef [n_steps, 4] = (dt, t, t_prev, 0); pattern_words [B, W],
 *   W = ceil(K / 32), the slot's visibility pattern in the bit layout of the attention's kmask (null: every key); mod_table [n_steps, R]
 *   and optionally mod_table_uncond [n_steps, R] (it and mods_uncond_out are null together); segs_host: n_segs <= 32 pairs (first column,
 *   width) on the HOST, ascending, widths multiples of 4 that tile the R columns exactly.  Writes
 *     kwords_out [B, W] = pattern_words[b] & bits(j < limit[step[b]]), bits at j >= K zero;
 *     coef_out [B, 4]   = (dt, t, t_prev, 1.0) of the slot's step;
 *     mods_out [B * R]  = row step[b] of the table, SEGMENT-MAJOR: segment s is the contiguous [B, width_s] slab at float offset B * first_s.
 *   An idle slot gets zero words, a zero coefficient row and the table's row 0.  1 <= K <= 2048, B <= 65535, 4 <= R <= 2^28.
 *
 * unpatchify_cfg_euler_rows: selftok_unpatchify_cfg_euler_f32 with dt = coef_rows[b][0] for every slot whose coef_rows[b][3] != 0 -- the
 *   same bits as that entry gives for the sample alone -- and step_out[b] = step[b] + 1; x0_param != 0: x_out = v + t_prev * (x - v) / t
 *   instead (v the CFG mix; fp32, uncontracted: difference, product, product with the fp32 reciprocal of t, sum).  A slot whose
 *   coef_rows[b][3] == 0 gets x_out[b] = x[b] byte for byte and step_out[b] = step[b]; nothing of y is read for it.  x_out == x and
 *   step_out == step are allowed.  y_uncond null: no CFG mix. */
int selftok_stream_prepare(const int* step, const int* limit, const float* coef, const unsigned* pattern_words, const float* mod_table,
                           const float* mod_table_uncond, const int* segs_host, int n_segs, unsigned* kwords_out, float* coef_out,
                           float* mods_out, float* mods_uncond_out, int B, int K, int n_steps, long R, hipStream_t stream);
int selftok_unpatchify_cfg_euler_rows_f32(const float* y_cond, const float* y_uncond, const float* x, float* x_out, const float* coef_rows,
                                          const int* step, int* step_out, int B, int C, int hp, int wp, float cfg_scale, int x0_param,
                                          hipStream_t stream);

/* ---- token statistics on [N, K] matrices of code ids (csrc/token_stats.hip) ----------------------------------------------------------
 * Code usage and perplexity, agreement of two tokenisations, the nearest sequence of a set.  Integer arithmetic, one fp64 entropy.  Every
 * entry is stateless and capturable, allocates and synchronises nothing, and decides every refusal on the host before any launch
 * (SELFTOK_EINVAL with a message; the workspace queries return 0 with the message set): a refused call leaves its outputs untouched.
 *
 * token_count: ids of id_bytes 2 (uint16), 4 (int32) or 8 (int64); id (r, k) sits at element r * row_stride + k * elem_stride (strides in
 *   ELEMENTS, >= 0).  counts[k * C + id] += 1 (uint32 [K, C], plain global atomics, accumulating: the caller zeroes once); an id outside
 *   [0, C) is not counted, writes nothing and adds 1 to bad[0].  n_rows * K and K * C below 2^31.  n_rows == 0: no launch.
 * token_census: counts [K, C] -> out double [K + 1, 5], one row per position and row K for the POOLED counts (the uint64 column sums over
 *   the positions): (n, used, H, H_ref, max_count), p = count / n, n the sum, used the codes with count > 0, H = -sum p ln p (a zero count
 *   adds exactly nothing), H_ref = -sum p ln(p + 1e-10).  fp64 in a fixed order (csrc/token_stats.hip states it), no atomics: the same
 *   bits every run.  A row with n == 0 is (0, 0, 0, 0, 0).  Workspace: the pooled counts, C * 8 bytes.
 * token_to_u16: the same ids -> dense uint16 out [n_rows, K]; an id outside [0, 65535] writes 0 and adds 1 to bad[0].
 * token_agree: a, b dense uint16 [n_rows, K], positions [k_lo, k_hi), 0 <= k_lo <= k_hi <= K <= 65535, n_rows <= 256 * 65535:
 *   match_pos[k] += 1 where the rows agree at k (uint32 [K], accumulating; positions outside the range untouched); per row n_diff, the
 *   lowest differing index first_diff (K if none) and the highest last_diff (-1 if none), all int32.
 * token_nearest: q [M, K], ref [N, K] dense uint16 -> best_match[i] = the largest number of equal positions in [k_lo, k_hi) over the
 *   reference rows, best_idx[i] = the lowest index that attains it (int32).  exclude_self == 0: every row is a candidate; exclude_self
 *   == 1 + o (o >= 0) skips j == i + o -- 1 for a set searched against itself, 1 + the chunk's first row when the queries are a chunk of
 *   it.  No candidate (N == 0, or the only row excluded): best_match -1, best_idx 0.  `split`: the number of reference splits (0 =
 *   automatic, clamped to min(64, ceil(N / 64))); the outputs never depend on it.  Workspace: one 64-bit key per split and query.
 *   M == 0 returns 0 without a launch. */
int selftok_token_count(const void* ids, int id_bytes, long n_rows, int K, int C, long row_stride, long elem_stride, unsigned* counts, unsigned* bad,
                        hipStream_t stream);
size_t selftok_token_census_workspace_bytes(int K, int C);
int selftok_token_census(const unsigned* counts, int K, int C, double* out, void* workspace, size_t workspace_bytes, hipStream_t stream);
int selftok_token_to_u16(const void* ids, int id_bytes, long n_rows, int K, long row_stride, long elem_stride, unsigned short* out, unsigned* bad,
                         hipStream_t stream);
int selftok_token_agree(const unsigned short* a, const unsigned short* b, int n_rows, int K, int k_lo, int k_hi, unsigned* match_pos, int* n_diff,
                        int* first_diff, int* last_diff, hipStream_t stream);
size_t selftok_token_nearest_workspace_bytes(int M, int N);
int selftok_token_nearest(const unsigned short* q, int M, const unsigned short* ref, int N, int K, int k_lo, int k_hi, int exclude_self, int split, int* best_match,
                          int* best_idx, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* ---- token sampler: AR logits over a window of C codes -> one code id per row (csrc/token_sample.hip) -------------------------------
 * Classifier-free guidance on the logits, temperature, top-k, top-p and one counter-based draw, reproducible bit for bit in numpy float32 /
 * uint64 (tests/token_sample_cases.py is that restatement): no library exponential, no floating-point sum whose order matters, no fused
 * multiply-add.  Stateless and capturable, no workspace, no synchronisation; every refusal is decided on the host before the launch
 * (SELFTOK_EINVAL with a message) and leaves the outputs untouched.  A row's outputs depend on that row's inputs alone.
 *
 * Inputs.  Row b of `logits` (and of `uncond_logits`, the same layout, or null) holds its window at elements b * row_stride + offset ..
 *   + C - 1; dtype 0 = fp32, 1 = bf16 (widened exactly).  1 <= C <= 65536, offset + C <= row_stride.  The pointers are aligned to four codes
 *   (16 bytes fp32, 8 bytes bf16), offset and (for B > 1) row_stride are multiples of 4.  ctr: uint32 [B, 2]; pos: int32 [B] or null.
 * 1. l = lu + s * (lc - lu), s = cfg_scale: difference, product, sum, each rounded to fp32; skipped when uncond_logits is null.  Then
 *    l = l * inv_T, inv_T = 1.0f / temperature computed once on the host.  temperature == 0 is GREEDY: inv_T = 1, the kept set is the first
 *    code of the order of (3), no random number is consumed.
 * 2. A row whose l holds a NaN or +inf, or nothing above -inf, is BAD: id -1, n_kept 0, masses 0, logprob NaN, bad[0] += 1, nothing else
 *    written.  (Guidance turns -inf in both inputs into NaN: mask codes with a large finite negative, or after the guidance.)  A row whose
 *    pos[b] lies outside [0, id_cols) is bad too, and its id is not written at all.
 * 3. Total order: l descending, index ascending on equal bits (a monotone uint32 key of l; -0.0 counts as +0.0).  Both filters keep a
 *    PREFIX of this order: ties are cut by index, never by chance.
 * 4. Integer mass, m the row maximum, d = l - m <= 0 in fp32: n = rint(d * 1.4426950408889634f); r = (d - n * 0.693145751953125f) -
 *    n * 1.428606765330187045e-06f; p = ((((((c6 r + c5) r + c4) r + c3) r + 1/2) r + 1) r + 1), c6 .. c3 = 1/720, 1/120, 1/24, 1/6 rounded
 *    to fp32, separate fp32 multiplies and adds; w = p * 2^(n + 32) (exact); q = (uint64) w (truncated); q = 0 for l = -inf or d < -24.  The
 *    maximum gets exactly 2^32; the relative error of w against exp is below 2^-21.  A code more than about 22.2 below the maximum has
 *    mass 0 and is never drawn.  Sums of up to 65536 masses stay below 2^49.
 * 5. top_k keeps the first min(k, C) codes of the order (k <= 0: off); their mass is Q_k.
 * 6. top_p, 0 < P < 1: T = (uint64) ceil((double) P * (double) Q_k); the kept set is the shortest prefix of the top-k prefix whose mass is
 *    >= T (at least one code).  P >= 1 or P <= 0: off.  Its mass is Q_kept.
 * 7. Draw: Philox4x32-10, key (seed_lo, seed_hi), counter (ctr[b][0], ctr[b][1], 0, 0); u = out[0] | out[1] << 32; r = mulhi64(u, Q_kept);
 *    the chosen code is the first kept code IN ASCENDING INDEX whose running mass exceeds r.
 * 8. Outputs: the id (0-based inside the window) as int32 / int64 (id_bytes 4 / 8) at element b * id_row_stride + (pos ? pos[b] : 0) of
 *    ids_out; n_kept[b] int32; mass[b] = (Q_total, Q_kept, q_id) uint64, Q_total the mass of the whole window; logprob[b] fp32 =
 *    ((double) l_id - (double) m) - log((double) Q_total * 2^-32), fp64 rounded once: the log-probability of the chosen code under the
 *    temperature-scaled UNFILTERED distribution.
 * B == 0 returns 0 without a launch. */
int selftok_sample_token(const void* logits, const void* uncond_logits, int dtype, int B, int C, long row_stride, long offset, float cfg_scale, float temperature,
                         int top_k, float top_p, unsigned seed_lo, unsigned seed_hi, const unsigned* ctr, const int* pos, void* ids_out, int id_bytes,
                         long id_row_stride, int id_cols, int* n_kept, unsigned long long* mass, float* logprob, unsigned* bad, hipStream_t stream);

/* ---- token scorer: AR logits over a window of C codes and a KNOWN id per row -> log-probability, rank, first code, entropy (csrc/token_score.hip) ----
 * The teacher-forced side of the sampler above, on the sampler's arithmetic: steps 1 - 4 of its text hold here word for word (guidance as difference,
 * product, sum; l * inv_T; the key and the total order "l descending, index ascending", -0.0 = +0.0; the integer mass q with the same constants, q = 0 for
 * d < -24, exactly 2^32 at the maximum), so that the two kernels can be held to each other by equality (tests/token_score_cases.py restates the rest in
 * numpy).  Stateless and capturable, no workspace, no synchronisation; every refusal is decided on the host before the launch (SELFTOK_EINVAL with a
 * message) and leaves the outputs untouched.  A row's outputs depend on that row's inputs alone.
 *
 * Inputs.  logits, uncond_logits, dtype, C, row_stride, offset, cfg_scale: the sampler's layout, alignment and window rules, R rows (R < 2^31, 64-bit
 *   element offsets).  temperature must be finite and > 0: a greedy distribution has no log-probabilities.  The target of row r is the int32 / int64
 *   (id_bytes 4 / 8) at element (r / S) * id_seq_stride + (r % S) * id_step_stride of `ids`, S = rows_per_seq >= 1, strides in ELEMENTS,
 *   id_step_stride possibly negative (the caller passes the base pointer already offset, and owns every element so addressed): rows of [B, S, V]
 *   logits in AR order score against [B, K] ids in tokenizer order without a flipped copy.  A target is 0-based inside the window.
 * Outputs, dense [R]:
 *   logprob fp32 = ((double) l_t - (double) m) - log((double) Q_total * 2^-32), rounded once: the sampler's formula.  A target more than 24 below the
 *     maximum has q_t = 0 and still a finite logprob; a target at -inf gets -inf.
 *   mass uint64 [R, 2] = (Q_total, q_t).
 *   rank int32 = the number of codes strictly ahead of the target in the total order (0: the target is what the sampler's greedy mode picks).
 *   top_id int32 = the first code of the order.
 *   entropy fp32, of the distribution the integer masses define: h_i = (uint64) trunc((double) q_i * (double) (-d_i) * 65536.0) for q_i > 0, else 0
 *     (two fp64 products, left to right); S_h = sum h_i, an integer sum (h_i < 2^47 since x e^-x <= 0.368, so S_h < 2^63 at C = 65536);
 *     H = log((double) Q_total * 2^-32) + (double) S_h / (65536.0 * (double) Q_total), fp64 rounded once.
 * Row kinds.  BAD: a NaN or +inf in l, nothing above -inf, or a target >= C: logprob NaN, rank -1, top_id -1, masses 0, entropy NaN, bad[0] += 1.
 *   IGNORED (the padding of a partial sequence): a target < 0 on a row that is not bad: logprob 0.0, rank -1, q_t 0; Q_total, top_id and entropy
 *   are written as for any row; ignored[0] += 1.  bad and ignored accumulate: the caller zeroes them.
 * R == 0 returns 0 without a launch. */
int selftok_score_tokens(const void* logits, const void* uncond_logits, int dtype, int R, int C, long row_stride, long offset, float cfg_scale, float temperature,
                         const void* ids, int id_bytes, int rows_per_seq, long id_seq_stride, long id_step_stride, float* logprob, unsigned long long* mass,
                         int* rank, int* top_id, float* entropy, unsigned* bad, unsigned* ignored, hipStream_t stream);

/* ---- token loss: AR logits over a window of C codes and a KNOWN id per row -> cross-entropy, log-sum-exp and the gradient row (csrc/token_xent.hip) ----
 * The training side of the scorer above, on its arithmetic at temperature 1 without guidance: l is the logit itself (l * 1.0f is exact), and steps 3 - 4 of
 * the sampler's text hold word for word (the key, -0.0 = +0.0, the row maximum m, the integer mass q_i with the same constants, q = 0 for d < -24, exactly
 * 2^32 at the maximum, Q_total their integer sum), so that nll is the scorer's logprob with the sign turned, bit for bit (tests/token_xent_cases.py restates
 * the rest in numpy).  Stateless and capturable, no workspace, no synchronisation; every refusal is decided on the host before the launch (SELFTOK_EINVAL
 * with a message) and leaves the outputs untouched.  A row's outputs depend on that row's inputs alone.
 *
 * Inputs.  logits, dtype, R, C, row_stride, offset, ids, id_bytes, rows_per_seq, id_seq_stride, id_step_stride: the scorer's layout, alignment, window and
 *   target-addressing rules.  V: the columns of a gradient row, offset + C <= V <= row_stride (and V <= grad_stride).  row_scale: fp32 dense [R] or null
 *   (1.0 for every row): the upstream scale g of the row -- weight / number of scored rows for a mean.  z_coef: finite, >= 0: the coefficient of the
 *   auxiliary term z_coef * lse^2.
 * Outputs.
 *   lse fp32 [R]: L = (double) m + log((double) Q_total * 2^-32), fp64; lse = (float) L, rounded once.
 *   nll fp32 [R] = (float) -(((double) l_t - (double) m) - log((double) Q_total * 2^-32)): the scorer's logprob with the sign bit turned (-0.0 where the
 *     logprob is +0.0).  A target more than 24 below the maximum has q_t = 0 and still a finite nll; a target at -inf among finite logits gets +inf and is
 *     NOT bad.
 *   grad, the logits' dtype, row r at element r * grad_stride, V columns written: column offset + i, i in [0, C), gets a * p_i - (i == t ? g : 0) with
 *     g = row_scale[r] (1.0f when null),
 *     a = g * (float) (1.0 + (2.0 * (double) z_coef) * L)   -- the fp64 product 2 z first, then that times L, then the sum, each rounded on its own, one
 *         rounding to fp32, one fp32 product; z_coef == 0 makes the factor exactly 1 and a == g,
 *     p_i = (float) ((double) q_i * (1.0 / (double) Q_total))   -- one fp64 quotient per row, one fp64 product and one rounding per code,
 *     the product a * p_i and the difference fp32, each rounded on its own (a column other than the target's subtracts +0.0, which changes no bit); bf16
 *     output is rounded to nearest even once (a NaN, which only a NaN or infinite row_scale produces, stays a NaN).  Columns [0, offset) and
 *     [offset + C, V) are written as +0; columns [V, grad_stride) are never touched.
 * Row kinds.  IGNORED: a target < 0 on a row that is not bad: nll +0.0, lse as for any row, the gradient row all +0 AND WRITTEN, ignored[0] += 1.
 *   BAD: a NaN or +inf logit in the window, nothing above -inf, or a target >= C: nll and lse NaN, bad[0] += 1, and the gradient row all +0 AND WRITTEN:
 *   the NaN in nll is what turns the trainer's loss into NaN, while zero gradients keep one poisoned row from destroying the other rows' buffers.
 *   bad and ignored accumulate: the caller zeroes them.
 * In place.  grad == logits with grad_stride == row_stride is allowed and gives the out-of-place bits: the logits are gone afterwards.  Any other
 *   intersection of the two extents (first to last addressed element of each) is refused.
 * R == 0 returns 0 without a launch. */
int selftok_xent_rows(const void* logits, int dtype, int R, int C, long row_stride, long offset, const void* ids, int id_bytes, int rows_per_seq,
                      long id_seq_stride, long id_step_stride, long V, const float* row_scale, float z_coef, float* nll, float* lse, void* grad,
                      long grad_stride, unsigned* bad, unsigned* ignored, hipStream_t stream);

/* ---- token distillation: STUDENT logits and TEACHER logits over one window of C codes -> KL(teacher || student), soft cross-entropy, teacher entropy,
 *      student log-sum-exp and the gradient row (csrc/token_distill.hip) ----
 * The full-distribution side of the loss above, on its arithmetic at temperature 1 on both sides: steps 3 - 4 of the sampler's text hold word for word for
 * EITHER row (the key, -0.0 = +0.0, the row maximum, the integer mass q_i with the same constants, q = 0 for d < -24, exactly 2^32 at the maximum, the
 * integer sum of the masses), and the teacher's entropy is the scorer's, bit for bit (tests/token_distill_cases.py restates the rest in numpy).  Stateless
 * and capturable, no workspace, no synchronisation; every refusal is decided on the host before the launch (SELFTOK_EINVAL with a message) and leaves the
 * outputs untouched.  A row's outputs depend on that row's inputs alone.
 *
 * Inputs.  student, dtype, R, C, row_stride, offset, V, row_scale, grad, grad_stride: the loss's layout, alignment, window and refusal rules.  teacher:
 *   teacher_dtype 0 = fp32, 1 = bf16, independent of the student's; row r holds the same window at elements r * teacher_stride + offset .. + C - 1; the
 *   pointer is aligned to four codes of ITS dtype and (for R > 1) teacher_stride is a multiple of 4.  teacher_uncond: null, or the teacher's dtype, stride
 *   and alignment; then the teacher logit is the sampler's step 1 word for word, a_i = lu + s * (lc - lu), s = cfg_scale (finite): difference, product,
 *   sum, each rounded to fp32; teacher is lc.  Otherwise a_i is the teacher's logit itself.  b_i is the student's logit.  row_scale: fp32 [R] or null
 *   (1.0).  row_mask: uint8 [R] or null; a 0 makes the row IGNORED.  grad: the student's dtype, or NULL: metrics only -- nothing of a gradient is written,
 *   V and grad_stride are not looked at.
 * Teacher: maximum mA, dA_i = a_i - mA (fp32), masses qA_i, sum QA.  Student: maximum mB, masses qB_i, sum QB.  LA = log((double) QA * 2^-32), LB likewise.
 * Outputs, fp32 dense [R], each one rounding of an fp64 value:
 *   lse_student = (float) ((double) mB + LB).
 *   h_teacher = (float) (LA + E_A), E_A = (double) S_A / (65536.0 * (double) QA), S_A = sum hA_i, hA_i = (uint64) trunc((double) qA_i * (double) (-dA_i) *
 *     65536.0) for qA_i > 0, else 0: the scorer's entropy of the teacher row.
 *   Cross term: x_i = (double) mB - (double) b_i, ONE fp64 subtraction of the two fp32 values (not the fp32 d the mass uses; the scorer's logprob is formed
 *     the same way); c_i = (uint64) trunc(((double) qA_i * x_i) * 65536.0) where qA_i > 0, else 0 (the fp64 product first, then the exact scaling, then the
 *     truncation).  A code with qA_i > 0 and x_i >= 32768.0 (+inf included: a student at -inf where the teacher has mass) sets the row's OVERFLOW flag and
 *     contributes c_i = 0.  S_lo = sum (c_i & 0xFFFFFFFF), S_hi = sum (c_i >> 32): two uint64 sums, each below 2^48 at 65536 codes, any order the same bits.
 *     X = (double) S_hi * 4294967296.0 + (double) S_lo; E_X = X / (65536.0 * (double) QA).
 *   ce = (float) (LB + E_X): the cross-entropy of the student under the teacher's distribution.
 *   kl = (float) (((LB - LA) + E_X) - E_A), not clamped at 0.  An OVERFLOW row gets ce = kl = +inf; it is NOT bad, and its gradient follows the formula.
 *   grad, row r at element r * grad_stride, V columns written: column offset + i gets g * (pB_i - pA_i), g = row_scale[r] (1.0f when null),
 *     pA_i = (float) ((double) qA_i * (1.0 / (double) QA)), pB_i likewise -- one fp64 quotient per row and side, one fp64 product and one rounding per code --
 *     the difference and the product fp32, each rounded on its own; bf16 output is rounded to nearest even once.  Columns [0, offset) and [offset + C, V)
 *     are written as +0; columns [V, grad_stride) are never touched.  This is the gradient of g * KL(teacher || student) with respect to the student logits.
 * Row kinds.  IGNORED (row_mask[r] == 0): the four outputs +0.0, the gradient row all +0 AND WRITTEN, ignored[0] += 1; no logit of the row is read.
 *   BAD, a row that is not ignored: a NaN or +inf in the window of student, teacher or teacher_uncond, or in the guided a_i (-inf in both teacher inputs
 *   gives NaN), or a_i or b_i with nothing above -inf: the four outputs NaN, the gradient row all +0 AND WRITTEN, bad[0] += 1.  NaN outside the window makes
 *   no row bad.  bad and ignored accumulate: the caller zeroes them.
 * In place.  grad == student with grad_stride == row_stride is allowed and gives the out-of-place bits: the student logits are gone afterwards.  Any other
 *   intersection of grad's extent with the student's (first to last addressed element of each), and ANY intersection with the extent of teacher or
 *   teacher_uncond, is refused.
 * R == 0 returns 0 without a launch. */
int selftok_distill_rows(const void* student, int dtype, const void* teacher, const void* teacher_uncond, int teacher_dtype, int R, int C, long row_stride,
                         long teacher_stride, long offset, float cfg_scale, long V, const float* row_scale, const unsigned char* row_mask, float* kl, float* ce,
                         float* h_teacher, float* lse_student, void* grad, long grad_stride, unsigned* bad, unsigned* ignored, hipStream_t stream);

/* ---- speculative token sampling: S drafted ids per sequence verified against the TARGET model's logits, the accepted prefix committed
 *      (csrc/token_verify.hip) ----
 * The accept / reject rule of speculative sampling on the sampler's integer arithmetic: masses are integers, sums are integer sums, both filters are
 * prefixes of one total order and every draw is counter-based, so the whole round is restated in numpy with Python integers
 * (tests/token_spec_cases.py) and, with draft logits equal to target logits, the emitted ids are bit for bit those of selftok_sample_token stepped
 * alone.  Two launches (verify, commit), capturable, no workspace, no synchronisation; every refusal is decided on the host before the first launch
 * (SELFTOK_EINVAL with a message) and leaves every buffer untouched.  A row's outputs depend on that row's inputs alone.
 *
 * Rows.  Row r = b * (S + 1) + s, sequence b in [0, B), slot s in [0, S]; 0 <= S <= 64.  The target row (b, s) holds its window at elements
 *   b * target_seq_stride + s * target_row_stride + offset .. + C - 1 of `target` (and of target_uncond, the same layout, or null); the draft row
 *   (b, s), s < S, likewise in `draft` / draft_uncond with the draft's strides.  Each side has its own dtype (0 = fp32, 1 = bf16), its own optional
 *   unconditional rows and its own scale (cfg_scale, draft_cfg_scale); temperature, top_k, top_p, the seed, C and offset are shared.  1 <= C <= 65536,
 *   offset + C <= either row stride; every logits pointer is aligned to four codes of its dtype, offset and every row and sequence stride are
 *   multiples of 4.  The drafted id x of row (b, s) is the int32 / int64 (draft_id_bytes 4 / 8) at element b * draft_id_stride + s of draft_ids, read
 *   only for s < n_draft[b]; a row with s >= n_draft[b], and a row whose id is negative, HAS NO DRAFT (x = -1): the bonus row s = n_draft[b] and any
 *   row past it.  n_draft: null (every sequence drafted S ids), or B counts given TWICE -- n_draft_host, host memory, checked here against
 *   0 <= n_draft[b] <= S, and n_draft, its device copy, which the kernels read (and clamp to [0, S]).  ctr: uint32 [B, 2], (ticket, step) of the
 *   sampler; row (b, s) uses the counter (ticket_b, step_b + s).
 * Both distributions.  Steps 1 - 6 of the sampler's text hold word for word for either row: guidance in separate roundings and l * inv_T, the bad-row
 *   rule, the total order, the integer mass relative to the row's OWN maximum, the top-k prefix, the top-p prefix.  p_i is the target mass of code i
 *   if i lies inside the target's kept set, else 0; P = sum p_i is the target's Q_kept.  d_i and D likewise for the draft.  Every mass is <= 2^32,
 *   every total < 2^49.  GREEDY (temperature 0): each kept set is the first code of its order, with mass 2^32; the rules below then say: accept iff x
 *   is the first code of both sides; the replacement is the target's first code.
 * Accept test (a row with a draft).  u32 = word 0 of Philox4x32-10(counter (ticket, step, 1, 0), key (seed_lo, seed_hi)).
 *   accept iff d_x > 0 and u32 * d_x * P < p_x * D * 2^32, both sides exact integers below 2^114 (128-bit products built from 64-bit multiplies and
 *   their high halves; no division, no floating point).  The acceptance probability is therefore min(1, p_x D / (d_x P)) ROUNDED UP to a multiple
 *   of 2^-32: ceil(2^32 p_x D / (d_x P)) of the 2^32 values of u32 accept (all of them once the ratio reaches 1).
 *   d_x == 0 is a FOREIGN draft id -- not drawn from this draft distribution: rejected, foreign[0] += 1; it is not a bad row.
 * Replacement (a rejected row with a draft).  w_i = (p_i * D - d_i * P) >> 34 where the 128-bit difference is positive, else 0.  p_i * D < 2^82, so
 *   w_i < 2^48; sum w_i <= sum p_i * D / 2^34 = P * D / 2^34 < 2^98 / 2^34 = 2^64: a uint64 sum never wraps.  Resolution: a residual below 2^34
 *   of the P * D scale -- a residual probability below 2^34 / (P D) <= 2^-30 (P, D >= 2^32) -- is dropped.  u64 = out[0] | out[1] << 32 of
 *   Philox(counter (ticket, step, 2, 0)); need = mulhi64(u64, sum w) + 1; the replacement is the first code IN ASCENDING INDEX whose running weight
 *   reaches need (the sampler's step 7 on the weights w).  sum w == 0 (x foreign while p and d are one distribution; never after an honest
 *   rejection): the row falls back to the draw below.
 * A row without a draft is the sampler's step 7 on p with the counter (ticket, step, 0, 0): the id, n_kept, Q_kept, the id's mass and the logprob of
 *   selftok_sample_token on that row, bit for bit.
 * BAD rows: a NaN or +inf in either side's l, nothing above -inf on either side (the draft's side only when the row has a draft), or x >= C:
 *   accept 0, repl_id -1, n_kept 0, the four masses 0, both logprobs NaN, bad[0] += 1.
 * Per-row outputs, dense [B * (S + 1)]: accept uint8; repl_id int32 (the replacement or the no-draft draw; -1 on an accepted and on a bad row);
 *   n_kept int32, the target's; mass uint64 [., 4] = (P, D, p_x, d_x) -- a row without a draft: (P, 0, the mass of the drawn code, 0); logprob_x
 *   and logprob_repl fp32: ((double) l_id - (double) m) - log((double) Q_total * 2^-32) of the TARGET row for x and for repl_id, the sampler's
 *   formula (NaN where there is no such id).  foreign and bad count over ALL B * (S + 1) rows and accumulate: the caller zeroes them.  Rows past
 *   the first rejection are computed and then discarded: every row is its own workgroup and none can know the prefix.
 * Commit, per sequence: n_accept[b] = the first s < n_draft[b] with accept 0, or n_draft[b]; n_emit[b] = max(0, min(n_accept[b] + 1, K - step_b)).
 *   For j < n_emit[b], tokenizer position K - 1 - (step_b + j) of row b of ids (int32 / int64, id_bytes), logprob_out and n_kept_out (row strides in
 *   elements, each >= K) receives: the drafted id, logprob_x and n_kept of row (b, j) for j < n_accept[b]; repl_id, logprob_repl and n_kept of row
 *   (b, n_accept[b]) for j == n_accept[b] (a bad row there commits id -1, NaN, 0, as the sampler does).  Then ctr[b][1] += n_emit[b].
 * B == 0 returns 0 without a launch. */
int selftok_verify_draft(const void* target, const void* target_uncond, int target_dtype, long target_seq_stride, long target_row_stride, const void* draft,
                         const void* draft_uncond, int draft_dtype, long draft_seq_stride, long draft_row_stride, const void* draft_ids, int draft_id_bytes,
                         long draft_id_stride, const int* n_draft_host, const int* n_draft, int B, int S, int C, long offset, float cfg_scale,
                         float draft_cfg_scale, float temperature, int top_k, float top_p, unsigned seed_lo, unsigned seed_hi, unsigned* ctr,
                         unsigned char* accept, int* repl_id, int* n_kept, unsigned long long* mass, float* logprob_x, float* logprob_repl, void* ids,
                         int id_bytes, long id_row_stride, int K, float* logprob_out, long logprob_row_stride, int* n_kept_out, long n_kept_row_stride,
                         int* n_accept, int* n_emit, unsigned* foreign, unsigned* bad, hipStream_t stream);

/* ---- token policy loss: AR logits over a window of C codes, a SAMPLED id per row, the log-probability it was drawn with and its advantage -> the clipped
 *      PPO / GRPO surrogate's coefficient, the k3 KL estimate to a reference, the entropy, and the gradient row (csrc/token_policy.hip) ----
 * The reinforcement-learning side of the loss above, on its arithmetic at temperature 1 without guidance: steps 3 - 4 of the sampler's text hold word for
 * word for m, d_i = l_i - m (fp32), q_i and Q (their integer sum); Lq = log((double) Q * 2^-32) (tests/token_policy_cases.py restates the rest in numpy).
 * Stateless and capturable, no workspace, no synchronisation; every refusal is decided on the host before the launch (SELFTOK_EINVAL with a message) and
 * leaves the outputs untouched.  A row's outputs depend on that row's inputs alone.
 *
 * Inputs.  logits, dtype, R, C, row_stride, offset, ids, id_bytes, rows_per_seq, id_seq_stride, id_step_stride, V, row_scale, grad, grad_stride: the loss's
 *   layout, alignment, window, in-place and refusal rules.  grad == NULL: metrics only -- nothing of a gradient is written, V and grad_stride are not looked
 *   at.  old_logprob, advantage: fp32 dense [R], required.  ref_logprob: fp32 dense [R] or null.  clip_lo, clip_hi, kl_coef, ent_coef: finite, >= 0,
 *   clip_lo < 1; kl_coef != 0 with a null ref_logprob is refused.  entropy: fp32 [R] or NULL (not wanted).
 * Per scored row, A = advantage[r], g = row_scale[r] (1.0f when null):
 *   lse = (float) ((double) m + Lq): the loss's.  lp = logprob = (float) (((double) l_t - (double) m) - Lq): the scorer's, bit for bit.
 *   ratio = (float) exp((double) lp - (double) old_logprob[r]): the difference is taken from the ROUNDED fp32 lp, so a roll-out scored by selftok_score_tokens
 *     or selftok_sample_token (temperature 1, unfiltered) gives a difference of exactly 0 and a ratio of exactly 1.0f.
 *   lo = 1.0f - clip_lo, hi = 1.0f + clip_hi (fp32).  clipped_hi = A > 0 && ratio > hi; clipped_lo = A < 0 && ratio < lo; flags[r] (uint8) = clipped_hi |
 *     clipped_lo << 1.  The surrogate is clipped_hi ? hi * A : clipped_lo ? lo * A : ratio * A, and +0 for A == 0 whatever the ratio (it is not an output: the
 *     host forms it from ratio, flags and A).
 *   kl: with a reference u = (double) ref_logprob[r] - (double) lp, e = expm1(u), kl = (float) (e - u): the k3 estimator exp(u) - u - 1, written so that a
 *     small u does not cancel.  Without a reference kl = +0 and e = 0.  (u = +inf -- a target at -inf under a finite reference -- gives inf - inf, a NaN kl.)
 *   entropy, the scorer's, bit for bit: S = sum (uint64) trunc((double) q_i * (double) (-d_i) * 65536.0) over q_i > 0, E = (double) S / (65536.0 * (double) Q),
 *     H = (float) (Lq + E).  S is formed only when ent_coef != 0 or entropy != NULL.
 *   coef[r] = k = g * (float) W, W = P + (double) kl_coef * e, P = (clipped_hi || clipped_lo || A == 0) ? 0.0 : (double) A * (double) ratio; each fp64
 *     operation rounded on its own.  k is minus the derivative of g * (-surrogate + kl_coef * kl) with respect to lp.
 *   grad, column offset + i: x_i = k * p_i - (i == t ? k : 0), p_i = (float) ((double) q_i * (1.0 / (double) Q)): selftok_xent_rows' formula with a = g = k,
 *     bit for bit.  With ent_coef != 0 the column gets x_i + kH * t_i instead (fp32 product, fp32 sum), kH = g * ent_coef (fp32), t_i = (float) (((double) q_i *
 *     (1.0 / (double) Q)) * ((double) d_i + E)) for q_i > 0, else +0: p_i (log p_i + H), the gradient of -H.  With ent_coef == 0 nothing is added (a -0.0
 *     stays -0.0).  bf16 output is rounded to nearest even once.  Columns [0, offset) and [offset + C, V) are written +0; [V, grad_stride) is never touched.
 * Row kinds.  IGNORED: a target < 0 on a row the loss would not call bad; its old_logprob, advantage and ref_logprob are not looked at: logprob, ratio, kl,
 *   entropy and coef +0, lse as for any row, flags 0, a gradient row of zeros WRITTEN, ignored[0] += 1.
 *   BAD: the loss's conditions (a NaN or +inf logit in the window, nothing above -inf, a target >= C); or, on a row with a target >= 0, a NaN or infinite
 *   advantage, a NaN or +inf old_logprob or ref_logprob, or a NaN difference (lp = -inf against an old_logprob or ref_logprob of -inf): every fp32 output
 *   NaN, flags 0, bad[0] += 1, a gradient row of zeros WRITTEN.  A target at -inf with a finite old_logprob is not bad: its ratio is 0.
 *   bad and ignored accumulate: the caller zeroes them.
 * In place.  grad == logits with grad_stride == row_stride is allowed and gives the out-of-place bits; any other intersection is refused.
 * R == 0 returns 0 without a launch. */
int selftok_policy_rows(const void* logits, int dtype, int R, int C, long row_stride, long offset, const void* ids, int id_bytes, int rows_per_seq,
                        long id_seq_stride, long id_step_stride, long V, const float* row_scale, const float* old_logprob, const float* advantage,
                        const float* ref_logprob, float clip_lo, float clip_hi, float kl_coef, float ent_coef, float* logprob, float* lse, float* ratio, float* kl,
                        float* entropy, float* coef, unsigned char* flags, void* grad, long grad_stride, unsigned* bad, unsigned* ignored, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SELFTOK_HIP_EXT_H */
