// Single-pass fp16 Linear on the split planes ("f16" GEMM mode):   out = act(fp16(A) fp16(W)^T + bias), fp32 accumulation
//
// The arithmetic of linear_f16x2_pre_kernel (gemm_split.hip) with both low planes taken as zero: fp16-rounded operands, ONE
// v_mfma_f32_32x32x16_f16 per product instead of three, fp32 accumulation.  A labelled, lossy mode (11 significand bits per
// operand) for bulk decoding -- not fp32-equivalent, and outside the 1e-3 dB of the fp32 / f16x2 modes.
//
// It reads the operands the f16x2 mode already holds and nothing else: the split activation [rows/16][K/32][plane][16][32]
// (only plane 0 of each 2-KiB chunk pair is fetched: the hi plane IS fp16(x)) and the packed weight image
// [N/128][K/32][hi|lo][k/8][128][8] (only the hi half of each 16-KiB tile).  No second packing, no second copy of the weights,
// half the LDS-DMA bytes and a third of the MFMAs of the f16x2 kernel.
//
// Contract with the f16x2 kernel, held by equality in tests/test_gemm_f16_gpu.py: every output is the ascending-k chain of 16-deep
// MFMA steps that the `hi` accumulator of linear_f16x2_pre_kernel executes, and the epilogue is that kernel's with lo = 0,
// operation for operation (hi + 0 + bias, GELU, split-activation output with BOTH planes, residual form resid + gate * y with two
// roundings, the range flag).  On operands that are fp16-representable the two kernels return the same numbers.
//
// Skeleton as linear_f16x2_pre_kernel: 256 x 128 output tile, 8 waves of 64 x 64, weights as the A operand of the MFMA (a lane
// owns an output row), both operands by LDS-DMA with the source-side XOR swizzle, XCD-aware tile order, ragged-M clamping of row
// blocks (the last chunk is read again, never past the tensor), ping-pong schedule of the two waves of a SIMD.  What differs is the
// staging: the freed LDS goes into 64-deep k-steps.  One ring stage holds TWO consecutive 32-deep k-tiles (2 x (16 KiB activation
// hi plane + 8 KiB weight hi half) = 48 KiB); three stages, filled two iterations ahead.  An iteration thus has 16 MFMAs per wave
// between two barriers (the f16x2 kernel: 24 per 32-deep tile) -- with 32-deep iterations it would have 8, and the barriers would
// cost as much as the matrix work.  Per iteration and wave: 16 fragment reads, 6 DMA pieces (4 activation + 2 weight), as before.
// K / 32 odd: the last stage's second half is staged from the last tile again (inside the tensor) and is not multiplied.
//
// The work-group -> tile map and the argument contract of the entry points are the f16x2 kernels' own: one definition each, in
// gemm_split_shared.h.
//
// Small row counts: by default the caller keeps rows <= SPLITK_MAX_ROWS on the f16x2 split-K route (ops.py, mmdit.py); the opt-in split-K
// form of this kernel is gemm_f16_splitk.hip (its own kernel text: this file's code object stays as it is).
#include "common.h"
#include "gemm_split_shared.h"
#include "selftok_hip_ext.h"

namespace selftok {

constexpr int H_A = PA_P;                          // 16384: hi plane of one 32-deep activation tile, [row 0..255][4 slots of 16 B]
constexpr int H_W = W_P;                           // 8192: hi half of one 32-deep weight tile, [k-group][n 0..127][8 halfs]
constexpr int H_W_BASE = 2 * H_A;                  // a stage: activation tiles 2 it, 2 it + 1, then weight tiles 2 it, 2 it + 1
constexpr int H_STAGE = 2 * (H_A + H_W);           // 49152
constexpr int H_STAGES = 3;
constexpr int H_LDS_BYTES = H_STAGES * H_STAGE;    // 147456 = the epilogue's transposition slices (8 waves x 2 planes x 64 x 144 B)

template <int ACT, int OSPLIT, int RES>
__global__ __launch_bounds__(512, 2) void linear_f16_pre_kernel(const _Float16* __restrict__ Ablk,
                                                                const _Float16* __restrict__ Wp, const float* __restrict__ bias,
                                                                float* __restrict__ out, _Float16* __restrict__ oblk, long ldo,
                                                                int M, int N, int K, int* __restrict__ overflow, int mblocks, int nblocks, ResArgs res)
{
    static_assert(!(OSPLIT && RES), "the residual form writes fp32");
    __shared__ __attribute__((aligned(16))) unsigned char smem[H_LDS_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: lives in an SGPR
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    int mb, nb;
    tile_of_workgroup(mblocks, nblocks, mb, nb);                    // gemm_split_shared.h
    const int m0 = mb * BM, n0 = nb * BN;
    const int KT = K / BK, KL = KT - 1;                             // 32-deep k-tiles of the operands
    const int NI = (KT + 1) >> 1, IL = NI - 1;                      // 64-deep iterations

    // ---- DMA maps: per 32-deep k-tile, wave w moves rows 16w..16w+15 and 128+16w.. of the activation hi plane (2 pieces) and 1 KiB
    // of the weight hi half (1 piece).  Sources are (uniform 64-bit base) + (per-lane 32-bit offset that never changes), LDS
    // destinations are scalar: issuing a piece costs scalar adds only ----
    const int d_g = (lane & 3) ^ ((lane >> 4) & 3);                 // source k-group of LDS slot (lane & 3) in row (lane >> 2)
    const unsigned a_off = (unsigned)((lane >> 2) * 64 + d_g * 16); // bytes inside a 1-KiB chunk [16 rows][32 halfs]: < 1024
    const int rb_last = (M - 1) >> 4;                               // ragged M: chunks past the end re-read the last one (rows discarded)
    int rb0 = m0 / 16 + wave, rb1 = rb0 + 8;
    rb0 = rb0 < rb_last ? rb0 : rb_last;
    rb1 = rb1 < rb_last ? rb1 : rb_last;
    // chunk (row block rb, k-tile kt, plane p) starts at ((rb KT + kt) 2 + p) KiB: plane 0 only
    const unsigned char* const a_base[2] = {(const unsigned char*)Ablk + (size_t)rb0 * KT * 2048, (const unsigned char*)Ablk + (size_t)rb1 * KT * 2048};
    // weight tile (nb, kt) starts at (nb KT + kt) 16 KiB: its first 8 KiB are the hi half, of which this wave moves KiB `wave`
    const unsigned char* const w_base = (const unsigned char*)Wp + (size_t)nb * KT * W_BYTES + (size_t)wave * 1024;
    const unsigned w_off = lane * 16;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    auto dma = [&](int it, int stage) {                             // 6 pieces: k-tiles 2 it and 2 it + 1
        const unsigned dst = lds0 + stage * H_STAGE + wave * 1024;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int kt = 2 * it + h;
            kt = kt < KL ? kt : KL;                                 // past the end: stage the last tile again (nobody multiplies it)
            lds_dma16(a_base[0] + (size_t)kt * 2048, a_off, dst + h * H_A);
            lds_dma16(a_base[1] + (size_t)kt * 2048, a_off, dst + h * H_A + 8192);
            lds_dma16(w_base + (size_t)kt * W_BYTES, w_off, dst + H_W_BASE + h * H_W);
        }
    };

    f32x16v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16v{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

    const int a_frag = (wm * 64 + l31) * PA_ROW + ((lh ^ ((l31 >> 2) & 3)) * 16);   // k-step 1: ^ 32 (k-group + 2); + b*32*64
    const int w_frag = H_W_BASE + lh * W_G + (wn * 64 + l31) * 16;                  // + b*32*16 + s*2*W_G
    f16x8 af[4][2], wf[4][2];                                       // fragments of the four 16-deep k-steps of an iteration
    auto read_frags = [&](int stage) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {                               // k-step q = tile half (q >> 1), 16-deep step (q & 1)
            const unsigned char* sa = smem + stage * H_STAGE + (q >> 1) * H_A + (a_frag ^ ((q & 1) * 32));
            const unsigned char* sw = smem + stage * H_STAGE + (q >> 1) * H_W + w_frag + (q & 1) * 2 * W_G;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                af[q][b] = *reinterpret_cast<const f16x8*>(sa + b * 32 * PA_ROW);
                wf[q][b] = *reinterpret_cast<const f16x8*>(sw + b * 32 * 16);
            }
        }
    };
    auto mfma_step = [&](int q) {                                   // weights as the A operand: lane = output row, registers = columns
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[q][j], af[q][i], acc[i][j], 0, 0, 0);
    };

    // ---- prologue: iterations 0 and 1 in flight; VM ops retire in issue order, so vmcnt(6) = the six pieces of iteration 0 landed ----
    dma(0, 0);
    dma(1, 1);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);

    // "Ping-pong" (see linear_f16x2_pre_kernel): the two waves of a SIMD (w and w + 4) run half an iteration apart; one issues its 16
    // MFMAs back to back while the other does all its memory work for its next iteration in their shadow.
    //   segment:   0      1      2      3     ...
    //   waves 0-3  L(0)   C(0)   L(1)   C(1)
    //   waves 4-7   -     L(0)   C(0)   L(1)       (one extra barrier up front, one less at the end)
    // Stage it % 3 is read in the load segments L(it) (segments 2 it and 2 it + 1, each closed by lgkmcnt(0) + barrier) and refilled
    // with iteration it + 3 by DMAs issued in L(it + 1) (segments 2 it + 2 / 2 it + 3).  Each wave waits for its own pieces of
    // iteration it + 1 at the end of L(it): they were issued in L(it - 1) and only this segment's six are younger -> vmcnt(6); the
    // barrier that follows makes them visible to the waves that read them in L(it + 1).
    const int grp = wave >> 2;
    if (grp) __builtin_amdgcn_s_barrier();
    if (grp) __builtin_amdgcn_s_setprio(1);                         // the later-dispatched half loses every issue arbitration otherwise
    int sc = 0;                                                     // it % 3
    for (int it = 0; it < NI; ++it) {
        const int s1 = sc == 2 ? 0 : sc + 1, s2 = s1 == 2 ? 0 : s1 + 1;
        __builtin_amdgcn_sched_barrier(0);
        read_frags(sc);
        __builtin_amdgcn_sched_barrier(0);
        dma(it + 2, s2);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        mfma_step(0);                                               // ascending k: steps 0, 1 of tile 2 it, then of tile 2 it + 1
        mfma_step(1);
        if (2 * it + 1 < KT) {                                      // wave-uniform: K / 32 odd has no second tile in its last iteration
            mfma_step(2);
            mfma_step(3);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!(grp && it == IL)) __builtin_amdgcn_s_barrier();
        sc = s1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // nothing of mine may still be writing LDS when the wave ends

    // ---- epilogue: linear_f16x2_pre_kernel's, with lo = 0.  D^T[n = (r&3) + 8 (r>>2) + 4 lh][m = l31] of each 32x32 block: a lane owns
    // one output row and, per register group, four consecutive columns; the wave's 64 x 64 outputs are transposed through its own
    // LDS slice (the ring is dead by now) and leave as 16 B per lane ----
    constexpr int STG_ROW = OSPLIT ? 144 : 272, STG_PLANE = 64 * STG_ROW;   // 64 rows x (128 | 256 B + pad); 18 | 17 KiB per wave
    static_assert(8 * (OSPLIT ? 2 * STG_PLANE : STG_PLANE) <= H_LDS_BYTES, "epilogue slices exceed the ring");
    unsigned char* stg = smem + wave * (OSPLIT ? 2 * STG_PLANE : STG_PLANE);
    __syncthreads();                                                // every wave has drained its DMAs (vmcnt(0) above): LDS is free
    float chk = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int cl = j * 32 + 8 * g + 4 * lh, col = n0 + wn * 64 + cl;
            const float4 bv = bias ? *reinterpret_cast<const float4*>(bias + col) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int rl = i * 32 + l31, row = m0 + wm * 64 + rl;
                float v[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    // `+ 0.f` is the f16x2 kernel's `+ lo * 2^-11` with lo = 0: it turns a -0 sum into +0 before the bias, as there
                    v[c] = acc[i][j][4 * g + c] + 0.f + (c == 0 ? bv.x : c == 1 ? bv.y : c == 2 ? bv.z : bv.w);
                    if (ACT == 1) v[c] = gelu_tanh_f(v[c]);
                }
                if (OSPLIT) {
                    f16x4 h, l;
                    split4(make_float4(opaque_f32(v[0]), opaque_f32(v[1]), opaque_f32(v[2]), opaque_f32(v[3])), h, l);   // common.h: why opaque
                    *reinterpret_cast<f16x4*>(stg + rl * STG_ROW + cl * 2) = h;
                    *reinterpret_cast<f16x4*>(stg + STG_PLANE + rl * STG_ROW + cl * 2) = l;
                    if (row < M) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) chk = __builtin_fmaf((float)h[c], 0.f, chk);   // |v| beyond fp16: h = inf -> flagged at the producer
                    }
                } else {
                    *reinterpret_cast<float4*>(stg + rl * STG_ROW + cl * 4) = make_float4(v[0], v[1], v[2], v[3]);
                    if (row < M) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) chk = __builtin_fmaf(v[c], 0.f, chk);
                    }
                }
            }
        }
    }
    if (OSPLIT) {                                                   // the slice is private to the wave: its LDS ops complete in order
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int pass = 0; pass < 8; ++pass) {
                const int rl = pass * 8 + (lane >> 3), seg = lane & 7, row = m0 + wm * 64 + rl;
                const f16x8 val = *reinterpret_cast<const f16x8*>(stg + p * STG_PLANE + rl * STG_ROW + seg * 16);
                if (row < M) *reinterpret_cast<f16x8*>(oblk + split_blk_index(row, n0 + wn * 64 + seg * 8, p, N / 32)) = val;
            }
    } else {
#pragma unroll
        for (int pass = 0; pass < 16; ++pass) {
            const int rl = pass * 4 + (lane >> 4), seg = lane & 15, row = m0 + wm * 64 + rl;
            float4 val = *reinterpret_cast<const float4*>(stg + rl * STG_ROW + seg * 16);
            if (row < M) {
                const int col = n0 + wn * 64 + seg * 4;
                if (RES) {
                    const float4 r = *reinterpret_cast<const float4*>(res.resid + (size_t)row * res.ldr + col);
                    if (res.gate) {
                        const int b = row / res.T, t = row - b * res.T;
                        const float4 g = *reinterpret_cast<const float4*>(res.gate + b * res.gsb + t * res.gst + col);
                        val.x = r.x + g.x * val.x; val.y = r.y + g.y * val.y; val.z = r.z + g.z * val.z; val.w = r.w + g.w * val.w;
                    } else {
                        val.x += r.x; val.y += r.y; val.z += r.z; val.w += r.w;
                    }
                }
                *reinterpret_cast<float4*>(out + (size_t)row * ldo + col) = val;
            }
        }
    }
    if (overflow && chk != 0.f) atomicOr(overflow, 1);
}

}  // namespace selftok

using namespace selftok;

extern "C" {

int selftok_linear_f16_split(const void* a_blk, const void* packed, const float* bias, float* out, void* out_blk, long ldo,
                             int M, int N, int K, int flags, int* overflow, hipStream_t stream)
{
    const int rc = check_split_linear("linear_f16_split", a_blk, packed, bias, out, out_blk, ldo, M, N, K);
    if (rc != SELFTOK_OK || M == 0) return rc;
    const bool osplit = out_blk != nullptr;
    const int mblocks = (M + BM - 1) / BM, nblocks = N / BN;
    const dim3 grid((unsigned)(mblocks * nblocks));
    const _Float16* ab = (const _Float16*)a_blk;
    _Float16* ob = (_Float16*)out_blk;
#define F16_LAUNCH(ACT, OS) hipLaunchKernelGGL((linear_f16_pre_kernel<ACT, OS, 0>), grid, dim3(512), 0, stream, ab, (const _Float16*)packed, bias, out, ob, ldo, M, N, K, overflow, mblocks, nblocks, ResArgs{})
    if (flags & SELFTOK_LINEAR_GELU) { if (osplit) F16_LAUNCH(1, 1); else F16_LAUNCH(1, 0); }
    else { if (osplit) F16_LAUNCH(0, 1); else F16_LAUNCH(0, 0); }
#undef F16_LAUNCH
    return check_launch("linear_f16_pre_kernel");
}

int selftok_linear_f16_split_residual(const void* a_blk, const void* packed, const float* bias,
                                      const float* resid, long ldr, const float* gate, long gate_stride_b, long gate_stride_t, int T,
                                      float* out, long ldo, int M, int N, int K, int* overflow, hipStream_t stream)
{
    const int rc = check_split_linear_residual("linear_f16_split_residual", a_blk, packed, bias, resid, ldr, gate, gate_stride_b, gate_stride_t, T, out, ldo, M, N, K);
    if (rc != SELFTOK_OK || M == 0) return rc;
    const int mblocks = (M + BM - 1) / BM, nblocks = N / BN;
    hipLaunchKernelGGL((linear_f16_pre_kernel<0, 0, 1>), dim3((unsigned)(mblocks * nblocks)), dim3(512), 0, stream,
                       (const _Float16*)a_blk, (const _Float16*)packed, bias, out, (_Float16*)nullptr, ldo,
                       M, N, K, overflow, mblocks, nblocks, ResArgs{resid, ldr, gate, gate_stride_b, gate_stride_t, T});
    return check_launch("linear_f16_pre_kernel(residual)");
}

}  // extern "C"
