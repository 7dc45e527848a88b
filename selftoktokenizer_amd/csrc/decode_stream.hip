// Decode stream (pipeline.DecodeStream): the two kernels of a sampler step in which every slot of the batch is at its OWN step.
//
//   stream_prepare_kernel        step[B] -> the slot's key-mask words, its (dt, t, t_prev, active) row and its rows of the
//                                modulation table(s), gathered segment-major so that every segment is the contiguous [B, width]
//                                tensor MMDiTGPU.core takes today.
//   unpatchify_euler_rows_kernel unpatchify + CFG mix + Euler update with one dt per slot; idle slots are copied byte for byte.
//
// Both are stateless, capturable, use no LDS, no atomics and no scratch; every refusal is decided on the host before a launch.
// The arithmetic of the velocity update is unpatchify_euler_kernel's (elementwise.hip), operation for operation.
#include "common.h"
#include "selftok_hip_ext.h"   // the C ABI declared there must match the definitions below

#pragma clang fp contract(off)

namespace selftok {

constexpr int STREAM_MAX_SEGS = 32;
constexpr int STREAM_CHUNK4 = 1024;      // float4 per workgroup: 256 lanes x 4 moves of 16 bytes, each move 4 KiB contiguous per workgroup

struct StreamSegs {
    int n;
    int first[STREAM_MAX_SEGS];
    int width[STREAM_MAX_SEGS];
};

__device__ __forceinline__ unsigned low_bits(int n)      // bits 0 .. n - 1 of a word (n <= 0: none, n >= 32: all)
{
    return n <= 0 ? 0u : (n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u));
}

// grid (chunks of R * tables, B), 256 threads.  Workgroup (0, b) also writes slot b's words and coefficient row.
__global__ __launch_bounds__(256) void stream_prepare_kernel(
    const int* __restrict__ step, const int* __restrict__ limit, const float* __restrict__ coef, const unsigned* __restrict__ pattern_words,
    const float* __restrict__ table0, const float* __restrict__ table1, StreamSegs segs,
    unsigned* __restrict__ kwords_out, float* __restrict__ coef_out, float* __restrict__ mods0_out, float* __restrict__ mods1_out,
    int B, int K, int W, int n_steps, int R4, int chunks)
{
    const int b = blockIdx.y;
    const int s = step[b];
    const bool active = s >= 0 && s < n_steps;
    const int row = active ? s : 0;                       // an idle slot reads row 0: finite modulations
    if (blockIdx.x == 0) {
        int lim = active ? limit[row] : 0;
        lim = lim < 0 ? 0 : (lim > K ? K : lim);
        for (int w = threadIdx.x; w < W; w += 256) {
            const unsigned pat = pattern_words ? pattern_words[(size_t)b * W + w] : 0xFFFFFFFFu;
            kwords_out[(size_t)b * W + w] = pat & low_bits(lim - 32 * w) & low_bits(K - 32 * w);
        }
        if (threadIdx.x == 0) {
            float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
            if (active) {
                c = *reinterpret_cast<const float4*>(coef + (size_t)row * 4);
                c.w = 1.0f;
            }
            *reinterpret_cast<float4*>(coef_out + (size_t)b * 4) = c;
        }
    }
    const int which = blockIdx.x / chunks, chunk = blockIdx.x - which * chunks;
    const float* __restrict__ src = (which ? table1 : table0) + (size_t)row * R4 * 4;
    float* __restrict__ dst = which ? mods1_out : mods0_out;
#pragma unroll
    for (int i = 0; i < STREAM_CHUNK4 / 256; ++i) {
        const int q = chunk * STREAM_CHUNK4 + i * 256 + threadIdx.x;      // float4 index inside the row
        if (q >= R4) break;
        const int col = q * 4;
        int first = 0, width = segs.width[0];
        for (int sg = 1; sg < segs.n; ++sg)                               // segments ascend and tile [0, R): the last one starting at or before `col`
            if (col >= segs.first[sg]) { first = segs.first[sg]; width = segs.width[sg]; }      // (a uniform index: scalar loads of the kernel argument)
        const size_t o = (size_t)B * first + (size_t)b * width + (col - first);
        *reinterpret_cast<float4*>(dst + o) = *reinterpret_cast<const float4*>(src + col);
    }
}

// one thread per output pixel pair, as unpatchify_euler_kernel.  coef_rows[b] = (dt, t, t_prev, active).
__global__ __launch_bounds__(256) void unpatchify_euler_rows_kernel(
    const float* __restrict__ y_cond, const float* __restrict__ y_uncond, const float* x, float* x_out,
    const float* __restrict__ coef_rows, const int* step, int* step_out, int B, int C, int hp, int wp, float cfg_scale, int x0_param)
{
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int Hh = 2 * hp, Ww = 2 * wp;
    const long per_slot = (long)C * Hh * wp;
    if (i >= (long)B * per_slot) return;
    int w = i % wp;
    long r = i / wp;
    int row = r % Hh; r /= Hh;
    int c = r % C;
    int b = r / C;
    const float4 cf = *reinterpret_cast<const float4*>(coef_rows + (size_t)b * 4);
    const bool active = cf.w != 0.0f;
    if (i - (long)b * per_slot == 0) {
        const int s = step[b];
        step_out[b] = active ? s + 1 : s;
    }
    size_t o = (((size_t)b * C + c) * Hh + row) * Ww + 2 * w;
    if (!active) {                                        // byte for byte (NaN payloads included); nothing of y is read
        if (x_out != x) *reinterpret_cast<uint2*>(x_out + o) = *reinterpret_cast<const uint2*>(x + o);
        return;
    }
    int h = row >> 1, p = row & 1;
    size_t tok = ((size_t)b * hp + h) * wp + w;
    const float* yc = y_cond + tok * (4 * C) + (p * 2) * C + c;
    float v0 = yc[0], v1 = yc[C];
    if (y_uncond) {
        const float* yu = y_uncond + tok * (4 * C) + (p * 2) * C + c;
        float u0 = yu[0], u1 = yu[C];
        v0 = u0 + cfg_scale * (v0 - u0);
        v1 = u1 + cfg_scale * (v1 - u1);
    }
    float2 xx = *reinterpret_cast<const float2*>(x + o);
    float2 out;
    if (x0_param) {
        // x_prev = v + t_prev * (x - v) / t as torch evaluates it on the device: the division by a host scalar is a
        // multiplication by its fp32 reciprocal; four roundings, none contracted
        const float inv_t = 1.0f / cf.y;
        const float a0 = cf.z * (xx.x - v0), a1 = cf.z * (xx.y - v1);
        out.x = v0 + a0 * inv_t;
        out.y = v1 + a1 * inv_t;
    } else {
        out.x = xx.x - cf.x * v0;
        out.y = xx.y - cf.x * v1;
    }
    *reinterpret_cast<float2*>(x_out + o) = out;
}

}  // namespace selftok

using namespace selftok;

extern "C" {

int selftok_stream_prepare(const int* step, const int* limit, const float* coef, const unsigned* pattern_words, const float* mod_table,
                           const float* mod_table_uncond, const int* segs_host, int n_segs, unsigned* kwords_out, float* coef_out,
                           float* mods_out, float* mods_uncond_out, int B, int K, int n_steps, long R, hipStream_t stream)
{
    if (!step || !limit || !coef || !mod_table || !segs_host || !kwords_out || !coef_out || !mods_out) {
        set_last_error("stream_prepare: null argument"); return SELFTOK_EINVAL;
    }
    if ((mod_table_uncond == nullptr) != (mods_uncond_out == nullptr)) {
        set_last_error("stream_prepare: the unconditional table and its output come together"); return SELFTOK_EINVAL;
    }
    if (B < 0 || B > 65535 || K < 1 || K > 2048 || n_steps < 1) {
        set_last_error("stream_prepare: expected 0 <= B <= 65535, 1 <= K <= 2048, n_steps >= 1"); return SELFTOK_EINVAL;
    }
    if (n_segs < 1 || n_segs > STREAM_MAX_SEGS) { set_last_error("stream_prepare: expected 1 .. 32 segments"); return SELFTOK_EINVAL; }
    if (R < 4 || R > (1L << 28) || (R & 3)) { set_last_error("stream_prepare: R must be a multiple of 4 in [4, 2^28]"); return SELFTOK_EINVAL; }
    StreamSegs segs;
    segs.n = n_segs;
    long at = 0;
    for (int s = 0; s < n_segs; ++s) {
        const int first = segs_host[2 * s], width = segs_host[2 * s + 1];
        if (width <= 0 || (width & 3)) { set_last_error("stream_prepare: a segment's width must be a positive multiple of 4"); return SELFTOK_EINVAL; }
        if (first != at) { set_last_error("stream_prepare: segments must ascend and tile the row without a gap"); return SELFTOK_EINVAL; }
        segs.first[s] = first; segs.width[s] = width;
        at += width;
    }
    if (at != R) { set_last_error("stream_prepare: the segment widths must sum to R"); return SELFTOK_EINVAL; }
    if (B == 0) return SELFTOK_OK;
    const int R4 = (int)(R / 4), W = (K + 31) / 32;
    const int chunks = (R4 + STREAM_CHUNK4 - 1) / STREAM_CHUNK4;
    hipLaunchKernelGGL(stream_prepare_kernel, dim3(chunks * (mod_table_uncond ? 2 : 1), B), dim3(256), 0, stream, step, limit, coef, pattern_words,
                       mod_table, mod_table_uncond, segs, kwords_out, coef_out, mods_out, mods_uncond_out, B, K, W, n_steps, R4, chunks);
    return check_launch("stream_prepare_kernel");
}

int selftok_unpatchify_cfg_euler_rows_f32(const float* y_cond, const float* y_uncond, const float* x, float* x_out, const float* coef_rows,
                                          const int* step, int* step_out, int B, int C, int hp, int wp, float cfg_scale, int x0_param,
                                          hipStream_t stream)
{
    if (!y_cond || !x || !x_out || !coef_rows || !step || !step_out) { set_last_error("unpatchify_cfg_euler_rows: null argument"); return SELFTOK_EINVAL; }
    if (B < 0 || C <= 0 || hp <= 0 || wp <= 0) { set_last_error("unpatchify_cfg_euler_rows: expected B >= 0 and C, hp, wp > 0"); return SELFTOK_EINVAL; }
    long total = (long)B * C * (2 * hp) * wp;
    if (total == 0) return SELFTOK_OK;
    if (total > 0x7FFFFFFFL * 256) { set_last_error("unpatchify_cfg_euler_rows: too many elements for one grid"); return SELFTOK_EINVAL; }
    hipLaunchKernelGGL(unpatchify_euler_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, y_cond, y_uncond, x, x_out, coef_rows,
                       step, step_out, B, C, hp, wp, cfg_scale, x0_param);
    return check_launch("unpatchify_euler_rows_kernel");
}

}  // extern "C"
