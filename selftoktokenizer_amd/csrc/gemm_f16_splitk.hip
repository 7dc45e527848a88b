// Split-K form of the single-pass fp16 Linear ("f16" GEMM mode, small row counts; opt-in: MMDiTGPU.set_gemm('f16', splitk='f16')).
//
// At one to four images (rows <= 1024) a 256 x 128 tile grid has 12 .. 192 work-groups for this model's Linears and each walks all of K
// alone.  Here gridDim.y = ksplit work-groups share an output tile, each over K / 32 / ksplit consecutive 32-deep k-tiles, and store their
// raw fp32 partial sums (no bias, no epilogue) to plane blockIdx.y of a [ksplit][M][N] workspace; the second launch is the f16x2 route's
// own splitk_finish_kernel (gemm_split.hip, reached through launch_splitk_finish of gemm_split_shared.h): planes added in ascending order,
// bias, GELU / split output / fused residual update.  LOSSY like its parent (fp16-rounded operands: DESIGN.md sections 22 and 26).
//
// Contract, held by equality in tests/test_gemm_f16_splitk_gpu.py: the partial of part s is the ascending chain of 16-deep MFMA steps over
// k-tiles s KT .. (s + 1) KT - 1 that the `hi` accumulator of linear_f16x2_pre_kernel<SK = 1> executes, stored as that kernel stores it with
// lo = 0 (hi + 0 + 0: a -0 sum leaves as +0), so with r = fp16 rounding
//     linear_f16_split_k(x, W, s) == linear_f16x2_split_k(r(x), r(W), s)        bit for bit.
//
// The k-loop is linear_f16_pre_kernel's (gemm_f16.hip), written out a second time so that that kernel's code object stays what it was
// ("Open"): hi planes only, both operands by LDS-DMA, ring of three 64-deep stages (two 32-deep k-tiles each) filled
// two iterations ahead, ping-pong schedule.  What differs: the operand bases start at this part's first k-tile, and the "past the end"
// clamp of the DMA is to the PART's last tile, never the tensor's.  Short chains (1, 2, 3 k-tiles: ksplit is chosen so that parts are
// short) need nothing else.  With KT k-tiles in the part, NI = ceil(KT / 2) iterations: the prologue stages iterations 0 and 1 and loop
// iteration `it` stages it + 2, every one of them 6 pieces per wave with the tile index clamped to KT - 1, so the vmcnt(6) accounting is
// the same for every NI >= 1 (12 pieces issued, the oldest 6 awaited; then 6 issued and 6 awaited per iteration) and a stage beyond the
// part holds the part's last tile again, which nobody multiplies.  KT odd: the last iteration multiplies its first half only.
#include "common.h"
#include "gemm_split_shared.h"
#include "selftok_hip_ext.h"

namespace selftok {

constexpr int HK_A = PA_P;                          // 16384: hi plane of one 32-deep activation tile, [row 0..255][4 slots of 16 B]
constexpr int HK_W = W_P;                           // 8192: hi half of one 32-deep weight tile
constexpr int HK_W_BASE = 2 * HK_A;                 // a stage: activation tiles 2 it, 2 it + 1, then weight tiles 2 it, 2 it + 1
constexpr int HK_STAGE = 2 * (HK_A + HK_W);         // 49152
constexpr int HK_LDS_BYTES = 3 * HK_STAGE;          // 147456: no more than linear_f16_pre_kernel

__global__ __launch_bounds__(512, 2) void linear_f16_splitk_partial_kernel(const _Float16* __restrict__ Ablk, const _Float16* __restrict__ Wp,
                                                                           float* __restrict__ ws, int M, int N, int K,
                                                                           int* __restrict__ overflow, int mblocks, int nblocks)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[HK_LDS_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: lives in an SGPR
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    int mb, nb;
    tile_of_workgroup(mblocks, nblocks, mb, nb);                    // gemm_split_shared.h: gridDim.x / blockIdx.x only
    const int m0 = mb * BM, n0 = nb * BN;
    const int KTA = K / BK;                                         // k-tiles of the operands (their strides)
    const int KT = KTA / (int)gridDim.y, KL = KT - 1;               // k-tiles of this work-group (the host checked the division)
    const int kt_off = (int)blockIdx.y * KT;
    const int NI = (KT + 1) >> 1, IL = NI - 1;                      // 64-deep iterations
    float* const out = ws + (size_t)blockIdx.y * M * N;             // this part's plane

    // ---- DMA maps: as linear_f16_pre_kernel, bases moved to k-tile kt_off ----
    const int d_g = (lane & 3) ^ ((lane >> 4) & 3);                 // source k-group of LDS slot (lane & 3) in row (lane >> 2)
    const unsigned a_off = (unsigned)((lane >> 2) * 64 + d_g * 16); // bytes inside a 1-KiB chunk [16 rows][32 halfs]: < 1024
    const int rb_last = (M - 1) >> 4;                               // ragged M: chunks past the end re-read the last one (rows discarded)
    int rb0 = m0 / 16 + wave, rb1 = rb0 + 8;
    rb0 = rb0 < rb_last ? rb0 : rb_last;
    rb1 = rb1 < rb_last ? rb1 : rb_last;
    // chunk (row block rb, k-tile kt, plane p) starts at ((rb KTA + kt) 2 + p) KiB: plane 0 only
    const unsigned char* const a_base[2] = {(const unsigned char*)Ablk + ((size_t)rb0 * KTA + kt_off) * 2048,
                                            (const unsigned char*)Ablk + ((size_t)rb1 * KTA + kt_off) * 2048};
    // weight tile (nb, kt) starts at (nb KTA + kt) 16 KiB: its first 8 KiB are the hi half, of which this wave moves KiB `wave`
    const unsigned char* const w_base = (const unsigned char*)Wp + ((size_t)nb * KTA + kt_off) * W_BYTES + (size_t)wave * 1024;
    const unsigned w_off = lane * 16;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    auto dma = [&](int it, int stage) {                             // 6 pieces: k-tiles 2 it and 2 it + 1 of the part
        const unsigned dst = lds0 + stage * HK_STAGE + wave * 1024;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int kt = 2 * it + h;
            kt = kt < KL ? kt : KL;                                 // past the PART's end: stage its last tile again (nobody multiplies it)
            lds_dma16(a_base[0] + (size_t)kt * 2048, a_off, dst + h * HK_A);
            lds_dma16(a_base[1] + (size_t)kt * 2048, a_off, dst + h * HK_A + 8192);
            lds_dma16(w_base + (size_t)kt * W_BYTES, w_off, dst + HK_W_BASE + h * HK_W);
        }
    };

    f32x16v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16v{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

    const int a_frag = (wm * 64 + l31) * PA_ROW + ((lh ^ ((l31 >> 2) & 3)) * 16);   // k-step 1: ^ 32 (k-group + 2); + b*32*64
    const int w_frag = HK_W_BASE + lh * W_G + (wn * 64 + l31) * 16;                 // + b*32*16 + s*2*W_G
    f16x8 af[4][2], wf[4][2];                                       // fragments of the four 16-deep k-steps of an iteration
    auto read_frags = [&](int stage) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {                               // k-step q = tile half (q >> 1), 16-deep step (q & 1)
            const unsigned char* sa = smem + stage * HK_STAGE + (q >> 1) * HK_A + (a_frag ^ ((q & 1) * 32));
            const unsigned char* sw = smem + stage * HK_STAGE + (q >> 1) * HK_W + w_frag + (q & 1) * 2 * W_G;
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

    // ping-pong of the two waves of a SIMD, half an iteration apart: see linear_f16_pre_kernel.  Barriers per wave: 2 NI either way
    // (waves 4-7: one up front, one less at the end), whatever NI.
    const int grp = wave >> 2;
    if (grp) __builtin_amdgcn_s_barrier();
    if (grp) __builtin_amdgcn_s_setprio(1);
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
        if (2 * it + 1 < KT) {                                      // wave-uniform: an odd part has no second tile in its last iteration
            mfma_step(2);
            mfma_step(3);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!(grp && it == IL)) __builtin_amdgcn_s_barrier();
        sc = s1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // nothing of mine may still be writing LDS when the wave ends

    // ---- store: linear_f16x2_pre_kernel<SK = 1>'s epilogue with lo = 0 and no bias -- v = hi + 0 + 0, transposed through the wave's own
    // LDS slice (the ring is dead by now), 16 B per lane, rows < M only; a non-finite partial raises the range flag as it does there ----
    constexpr int STG_ROW = 272, STG_PLANE = 64 * STG_ROW;          // 64 rows x (256 B + pad): 17 KiB per wave
    static_assert(8 * STG_PLANE <= HK_LDS_BYTES, "store slices exceed the ring");
    unsigned char* stg = smem + wave * STG_PLANE;
    __syncthreads();                                                // every wave has drained its DMAs (vmcnt(0) above): LDS is free
    float chk = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int cl = j * 32 + 8 * g + 4 * lh;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int rl = i * 32 + l31, row = m0 + wm * 64 + rl;
                float v[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = acc[i][j][4 * g + c] + 0.f + 0.f;     // `+ lo * 2^-11` with lo = 0, `+ bias` with none
                *reinterpret_cast<float4*>(stg + rl * STG_ROW + cl * 4) = make_float4(v[0], v[1], v[2], v[3]);
                if (row < M) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) chk = __builtin_fmaf(v[c], 0.f, chk);
                }
            }
        }
    }
#pragma unroll
    for (int pass = 0; pass < 16; ++pass) {                         // the slice is private to the wave: its LDS ops complete in order
        const int rl = pass * 4 + (lane >> 4), seg = lane & 15, row = m0 + wm * 64 + rl;
        const float4 val = *reinterpret_cast<const float4*>(stg + rl * STG_ROW + seg * 16);
        if (row < M) *reinterpret_cast<float4*>(out + (size_t)row * N + n0 + wn * 64 + seg * 4) = val;
    }
    if (overflow && chk != 0.f) atomicOr(overflow, 1);
}

// first launch of a split-K Linear in the f16 mode: the partial planes
static int launch_f16_partials(const void* a_blk, const void* packed, float* ws, int M, int N, int K, int ksplit, int* overflow, hipStream_t stream)
{
    const int mblocks = (M + BM - 1) / BM, nblocks = N / BN;
    hipLaunchKernelGGL(linear_f16_splitk_partial_kernel, dim3((unsigned)(mblocks * nblocks), (unsigned)ksplit), dim3(512), 0, stream,
                       (const _Float16*)a_blk, (const _Float16*)packed, ws, M, N, K, overflow, mblocks, nblocks);
    return check_launch("linear_f16_splitk_partial_kernel");
}

}  // namespace selftok

using namespace selftok;

extern "C" {

int selftok_linear_f16_split_k(const void* a_blk, const void* packed, const float* bias, float* out, void* out_blk, long ldo,
                               int M, int N, int K, int flags, int ksplit, void* workspace, int* overflow, hipStream_t stream)
{
    if (ksplit == 1) return selftok_linear_f16_split(a_blk, packed, bias, out, out_blk, ldo, M, N, K, flags, overflow, stream);
    int rc = check_split_linear("linear_f16_split_k", a_blk, packed, bias, out, out_blk, ldo, M, N, K);
    if (rc != SELFTOK_OK || M == 0) return rc;
    if ((rc = check_splitk("linear_f16_split_k", K, ksplit, workspace))) return rc;
    float* ws = (float*)workspace;
    if ((rc = launch_f16_partials(a_blk, packed, ws, M, N, K, ksplit, overflow, stream))) return rc;
    return launch_splitk_finish(ws, ksplit, bias, out, out_blk, ldo, M, N, flags, overflow, nullptr, stream);
}

int selftok_linear_f16_split_residual_k(const void* a_blk, const void* packed, const float* bias,
                                        const float* resid, long ldr, const float* gate, long gate_stride_b, long gate_stride_t, int T,
                                        float* out, long ldo, int M, int N, int K, int ksplit, void* workspace, int* overflow, hipStream_t stream)
{
    if (ksplit == 1)
        return selftok_linear_f16_split_residual(a_blk, packed, bias, resid, ldr, gate, gate_stride_b, gate_stride_t, T, out, ldo, M, N, K, overflow, stream);
    int rc = check_split_linear_residual("linear_f16_split_residual_k", a_blk, packed, bias, resid, ldr, gate, gate_stride_b, gate_stride_t, T, out, ldo, M, N, K);
    if (rc != SELFTOK_OK || M == 0) return rc;
    if ((rc = check_splitk("linear_f16_split_residual_k", K, ksplit, workspace))) return rc;
    float* ws = (float*)workspace;
    if ((rc = launch_f16_partials(a_blk, packed, ws, M, N, K, ksplit, overflow, stream))) return rc;
    const ResArgs res{resid, ldr, gate, gate_stride_b, gate_stride_t, T};
    return launch_splitk_finish(ws, ksplit, bias, out, nullptr, ldo, M, N, 0, overflow, &res, stream);
}

}  // extern "C"
